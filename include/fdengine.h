/*
 * fdengine.h — C-ABI of the MI355X-native fraud-scoring engine (libfdengine.so).
 *
 * The engine is the drop-in for ONE hot path of AjayAlluri/realtime-fraud-detection:
 *   windowed per-card features -> XGBoost primary classifier + Isolation Forest anomaly score
 *   -> ensemble blend / decision.
 *
 * Every entry point below replaces a named reference interface (paths relative to the
 * reference repo root; "ml/" = services/ml-models/src/, "fl/" = services/flink-jobs/src/main/
 * java/com/frauddetection/).  The Python host shim (realtime-fraud-detection_amd/fdengine/)
 * binds these with ctypes; INTEGRATION.md shows the binding a maintainer adds.
 *
 * Conventions (mirroring ml/models/model_manager.py:279-307):
 *   - every function returns int status, FD_OK == 0; nothing throws across the ABI;
 *   - fd_last_error() returns a thread-local message for the last failure on this thread;
 *   - caller-owned buffers; "_device" functions take device pointers (HBM-resident inputs),
 *     "_host" functions take host pointers and are synchronous;
 *   - one engine per GPU; every entry point taking an engine holds that engine's (recursive) lock, so
 *     calls from several host threads are serialised per engine (the reference serialises on one
 *     asyncio loop, ml/main.py:337-344; here ModelManager.predict runs in a worker thread beside the
 *     loop's own calls). fd_engine_destroy while another thread still uses the engine is undefined.
 * No PyTorch / HIP types appear in these signatures; streams are passed as void*.
 */
#ifndef FDENGINE_H
#define FDENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FD_ABI_VERSION 15

enum fd_status {
  FD_OK = 0,
  FD_ERR_INVALID_ARG = 1,
  FD_ERR_HIP = 2,
  FD_ERR_NOT_LOADED = 3, /* ValueError("Model ... not loaded"), ml/models/model_manager.py:281-282 */
  FD_ERR_UNSUPPORTED = 4,
  FD_ERR_OOM = 5,
  FD_ERR_IO = 6, /* snapshot file missing / truncated / corrupt (checksum) */
};

/* Forest kinds: the tree model types on the path. */
enum fd_forest_kind {
  /* xgboost 2.0.3 gbtree, objective binary:logistic
     (ml/models/model_manager.py:157-161 load, :309-311 predict_proba[:,1]) */
  FD_FOREST_XGB_BINARY_LOGISTIC = 1,
  /* scikit-learn IsolationForest, decision_function then 1/(1+e^s)
     (ml/models/model_manager.py:197-200 load, :338-346 predict) */
  FD_FOREST_SKLEARN_IFOREST = 2,
  /* scikit-learn RandomForestClassifier / ExtraTreesClassifier / DecisionTreeClassifier, two classes:
     predict_proba(X)[:, 1] (ml/models/model_manager.py:338-346, the branch for models with predict_proba).
     Comparison and NaN rules are sklearn's, as for the IsolationForest (default_left = missing_go_to_left);
     leaf_value = tree_.value[node, 0, 1] (f64); raw = the f64 sum of the leaf values in tree order,
     prob = raw / n_trees. Served by the sparse layout only (fd_pack_forest_sparse_host). */
  FD_FOREST_SKLEARN_PROBA = 3,
};

typedef struct fd_engine fd_engine;

/* Original (un-repacked) tree arrays of one forest, concatenated over trees.
   Node ids are per tree, 0-based, exactly as the source library numbers them
   (XGBoost JSON `left_children`/... arrays; sklearn `tree_.children_left`/...). */
typedef struct {
  int32_t n_trees;
  const int64_t* tree_offsets; /* n_trees+1 offsets into the node arrays */
  const int32_t* left;         /* left child, -1 marks a leaf */
  const int32_t* right;        /* right child */
  const int32_t* feature;      /* split column in the caller's feature matrix */
  const double* threshold;     /* split value as the library stores it (XGB: f32 value; sklearn: f64) */
  const uint8_t* default_left; /* missing-value (NaN) direction; NULL = right */
  const double* leaf_value;    /* per node, read at leaves (XGB: leaf weight; IF: depth+c(n)-1) */
} fd_tree_arrays;

typedef struct {
  int32_t kind;        /* enum fd_forest_kind */
  int32_t num_feature; /* model columns (XGB learner_model_param.num_feature / sklearn n_features_in_) */
  double base_score;   /* XGB: learner_model_param.base_score (probability space) */
  double if_offset;    /* IF: offset_ */
  double if_denominator; /* IF: n_estimators * _average_path_length([max_samples]) */
} fd_forest_params;

/* Ensemble blend parameters (ml/models/ensemble_predictor.py:62-73, 252-369). Models are listed
   in the reference's enabled-model order (ml/utils/config.py:128-199). */
#define FD_MAX_MODELS 8
enum fd_blend_strategy { FD_BLEND_WEIGHTED_AVERAGE = 0, FD_BLEND_VOTING = 1, FD_BLEND_STACKING = 2 };
enum fd_decision { FD_APPROVE = 0, FD_REVIEW = 1, FD_DECLINE = 2, FD_APPROVE_WITH_MONITORING = 3 };
enum fd_risk { FD_VERY_LOW = 0, FD_LOW = 1, FD_MEDIUM = 2, FD_HIGH = 3, FD_CRITICAL = 4 };
typedef struct {
  int32_t n_models;
  int32_t strategy;                  /* enum fd_blend_strategy */
  double weight[FD_MAX_MODELS];      /* normalised weights, _get_model_weights :62-73 */
  double conf_mult[FD_MAX_MODELS];   /* _calculate_model_confidence multipliers :331-337 */
  double fraud_threshold;            /* EnsembleConfig.fraud_threshold (0.5) */
  double confidence_threshold;       /* EnsembleConfig.confidence_threshold (0.7) */
} fd_blend_params;

/* ---------------------------------------------------------------- engine lifecycle */
const char* fd_last_error(void);
int fd_abi_version(void);
/* "fdengine-build-id:src=<digest>;flags=<hipcc flags>": SHA-256 (first 128 bits) of the HIP sources, the csrc
   headers and this header the library was built from (fdengine/_buildid.py); the Python loader refuses a
   library whose digest differs from the tree beside it. */
const char* fd_build_id(void);
int fd_device_count(int* out);
/* ModelManager.__init__ (ml/models/model_manager.py:33-45): one engine per GPU. */
int fd_engine_create(int device, fd_engine** out);
int fd_engine_destroy(fd_engine* eng);
/* Launch on a caller stream (hipStream_t as void*). NULL is the device's null (default) stream,
   e.g. PyTorch's default stream, whose handle is 0. fd_engine_reset_stream restores the engine's
   own non-blocking stream. */
int fd_engine_set_stream(fd_engine* eng, void* hip_stream);
int fd_engine_reset_stream(fd_engine* eng);
int fd_engine_sync(fd_engine* eng);

/* ---------------------------------------------------------------- forests (a8, a9) */
/* Replaces _load_xgboost_model (ml/models/model_manager.py:157-161) and _load_sklearn_model
   (:197-200): repacks the original trees into the engine's depth-major layout and uploads them. */
int fd_load_forest(fd_engine* eng, int slot, const fd_forest_params* params, const fd_tree_arrays* trees);
int fd_unload_forest(fd_engine* eng, int slot);

/* Load the reference's XGBoost model FILE unchanged into `slot` (replaces ModelManager._load_xgboost_model,
   services/ml-models/src/models/model_manager.py:157-161: XGBClassifier().load_model(path); the file is
   XGBClassifier.save_model's XGBoost 2.0.3 JSON, model_trainer.py:95-108). Parsed in C++ — a C / C++ / JNI
   host needs no Python — then repacked exactly as fd_load_forest. FD_ERR_IO: unreadable file;
   FD_ERR_UNSUPPORTED: objective other than binary:logistic, booster other than gbtree, multi-class,
   categorical splits or vector leaves; FD_ERR_INVALID_ARG: malformed JSON / tree arrays. */
int fd_load_xgboost_json(fd_engine* eng, int slot, const char* path);

/* Host-only (no device): the same file flattened into caller arrays, the parity hook for the reader.
   Call with trees == NULL to get *n_trees / *n_nodes, then with trees' arrays sized n_trees + 1 (offsets)
   and n_nodes (the rest); params receives kind, num_feature and base_score. */
int fd_xgboost_json_read(const char* path, fd_forest_params* params, int32_t* n_trees, int64_t* n_nodes,
                         fd_tree_arrays* trees);
int fd_forest_info(fd_engine* eng, int slot, int32_t* n_trees, int32_t* depth, int32_t* num_feature);

/* Replaces _predict_xgboost (:309-311) / _predict_sklearn (:338-346) for a batch.
   d_X: n x ld row-major f32 (what XGBoost's DMatrix / sklearn's validate_data cast the f64 vector to).
   d_prob: P(fraud) per row (XGB: f32 sigmoid widened; IF: 1/(1+exp(decision_function)); sklearn classifier:
   predict_proba[:, 1]).
   d_raw (optional): XGB margin / IF summed path length / classifier: summed leaf values.
   d_leaf (optional): n x n_trees original leaf node ids (xgboost pred_leaf / sklearn apply). */
int fd_forest_predict_device(fd_engine* eng, int slot, const float* d_X, int64_t n, int32_t ld,
                             double* d_prob, double* d_raw, int32_t* d_leaf);
int fd_forest_predict_host(fd_engine* eng, int slot, const float* X, int64_t n, int32_t ld,
                           double* prob, double* raw, int32_t* leaf);

/* Host-only repack (no device needed): the layouts fd_load_forest uploads, for layout inspection
   and CPU tests. Call with NULL buffers to query sizes in *info.
   fd_pack_forest_host: threshold layout — per tree a 1-based heap of 2^D {f32 thr, u32 meta}
   records (slot 0 unused, children of slot s at 2s / 2s+1) then 2^D leaf values.
   fd_pack_forest_binned_host: binned layout — every split threshold replaced by its index j in the
   feature's sorted table of distinct thresholds (x < t_j  <=>  bin(x) <= j, bin(x) = #{t <= x}), so a
   node is one u32 (j << 16 | feature * 1024 | default_left); 2^D node words then 2^D leaf values.
   Returns FD_ERR_UNSUPPORTED when a feature has more than 65534 distinct thresholds. */
typedef struct {
  int32_t n_trees;
  int32_t n_chunks;
  int32_t chunk;        /* trees per LDS staging chunk */
  int32_t depth;        /* D: every tree is padded to a perfect depth-D tree */
  int64_t tree_bytes;   /* 2^D node records (8 B threshold layout / 4 B binned) + 2^D leaf values
                           (f32 XGB / f64 IF) */
  int64_t chunk_stride; /* bytes per chunk, 1 KiB multiple */
  int64_t blob_bytes;
  int64_t n_leaf_ids;
  float base_margin;    /* XGB: f32 margin seeded by base_score */
  int32_t layout;       /* 0 threshold layout, 1 binned layout */
  int64_t n_thresholds; /* binned: total distinct thresholds over all features */
  int32_t bin_steps;    /* binned: largest power of two <= the longest feature table (0 if none) */
} fd_pack_info;
int fd_pack_forest_host(const fd_forest_params* params, const fd_tree_arrays* trees, void* blob,
                        int64_t blob_cap, int32_t* leaf_ids, int64_t ids_cap, fd_pack_info* info);
/* thresholds: n_thresholds f32 (feature-major, ascending per feature); offsets: num_feature + 1. */
int fd_pack_forest_binned_host(const fd_forest_params* params, const fd_tree_arrays* trees, void* blob,
                               int64_t blob_cap, float* thresholds, int64_t thr_cap, int32_t* offsets,
                               fd_pack_info* info);

/* Host-only: the forest contracted against the constant slots of the compact scoring vector. The pipelined stream's
   compact and split rows carry 22 varying slots; of the other 42, slots 12, 24, 25, 33 and 34 are always 0.5 and the
   rest 0 (the reference's feature map at serving time). Every split on such a slot is replaced by the child that value
   takes (left iff value < threshold in f32, the packers' comparison; never NaN, so default_left plays no part), which
   is what the fused kernel walks on those rows (engine option ensemble_contract). Surviving nodes keep their order
   (a tree with no such split comes back unchanged); a tree that resolves to one leaf becomes a root over two leaves
   of that value. XGBoost and IsolationForest kinds.
   Call with out == NULL for *n_nodes, then with out's arrays sized n_trees + 1 (offsets) and *n_nodes (the rest).
   depths (optional, n_trees): each contracted tree's depth, at least 1; n_pruned (optional): splits removed. */
int fd_contract_forest_host(const fd_forest_params* params, const fd_tree_arrays* trees, int64_t* n_nodes,
                            fd_tree_arrays* out, int32_t* depths, int64_t* n_pruned);

/* Host-only: the dense chunk layout of one contracted forest, as the fused kernel walks it on compact / split rows
   under ensemble_contract 3 and 4 (the engine's plan is built by the same function, against the two forests' merged
   threshold tables; here the tables are the forest's own). XGBoost and IsolationForest kinds, contracted depth <= 8.
   Bundles: trees_per_bundle trees walked by one wave (wide 6 XGBoost / 4 IsolationForest, compact 5 / 3), every tree
   of a bundle a perfect 1-based heap of the bundle's depth d = the deepest of its trees. mode 3: tree i of the forest
   in bundle i / trees_per_bundle; mode 4: the chunk's trees sorted by depth (deepest first, forest order among
   equals), then cut into bundles, a partial bundle (the forest's last chunk) at the last
   place where the sum of the walked depths is least. A chunk is a run of consecutive trees, grown a bundle's worth of trees at a time
   while it holds at most s_max bundles and its data fit buf_bytes. Its bundles go to the four tree groups deepest
   first, each to the group with the least sum of depths so far (the lowest group on ties; group 0 starts at
   owner_bias / 16 levels per tree of the chunk, 0 = none).
   Chunk image: node blocks (largest first), then leaf rows (forest order), zero-padded to 1 KiB; then the 1 KiB chunk
   table. A tree's node block is 4 * 2^d bytes, aligned to its size: word s (1 <= s < 2^d) is heap slot s,
     threshold index << 16 | (slot >> 1) << 10 | link << 3 | (slot & 1) << 1 | default_left
   slot = the feature's index among the 22 varying slots (0, 1, 5, 6, 7, 14, 15, 16, 17, 19, 21, 23, 26, 27, 31, 32,
   41..46), threshold index j into the feature's ascending table: left iff bin(x) <= j, bin(x) = #{t <= x}, NaN:
   default_left. link = s above the last split level (the children are words 2 s, 2 s + 1), s - 2^(d-1) on it: the leaf
   index is 2 link + right. A node below a leaf is a pad (threshold index 0, slot 0): both ways reach that leaf's
   value. Its leaf row is 2^d values (f32 XGBoost, f64 IsolationForest). The free slots of a partial last bundle repeat
   its first tree's block. Chunk table, u32 words: [0] trees | bundles << 8; [1], [2] the next chunk's offset and
   length in KiB (0, 0 after the last); [3] bundles of tree group g in byte g; at byte 64 + 128 g + 16 i the i-th
   bundle of group g: {d | bundle << 8 | g << 16, then six u16 node-block offsets}; at byte 576 + 4 k the chunk's k-th
   tree (forest order): leaf-index byte (2048 bundle + place in the bundle) | leaf-row offset << 16.
   Call with blob == NULL for info, then with blob (info->blob_bytes), chunk_offsets / chunk_lengths (info->n_chunks),
   tree_info (n_trees), thresholds (info->n_thresholds) and thr_offsets (num_feature + 1); any may be NULL. */
typedef struct fd_dense_tree {
  int32_t chunk, bundle, group, depth;  /* bundle: index in its chunk; depth: as walked */
  int32_t node_offset, leaf_offset;     /* bytes from the chunk's start */
} fd_dense_tree;
typedef struct fd_dense_info {
  int32_t n_chunks, s_max, trees_per_bundle, buf_bytes;
  int64_t blob_bytes, n_thresholds, node_steps; /* node_steps: the sum of the trees' walked depths */
} fd_dense_info;
int fd_dense_layout_host(const fd_forest_params* params, const fd_tree_arrays* trees, int32_t wide, int32_t mode,
                         int32_t owner_bias, fd_dense_info* info, void* blob, int64_t* chunk_offsets,
                         int32_t* chunk_lengths, fd_dense_tree* tree_info, float* thresholds, int32_t* thr_offsets);

/* Sparse (pointer) layout, host-only repack: trees of ANY depth and any kind keep their shape (no padding). It is the
   only layout of FD_FOREST_SKLEARN_PROBA and of forests deeper than 10 levels (fd_load_forest picks it for them;
   fd_forest_info then reports the true depth), and what engine option forest_kernel = 11 walks for any forest.
     nodes: n_nodes records of 8 bytes {f32 t, u32 meta}, "go left <=> x < t" (sklearn's (double)x <= thr rewritten
       as for the other layouts). Records 0 .. n_trees-1 are the roots in tree order; behind them each tree's other
       nodes in breadth-first order, so a node's two children are adjacent records.
       internal node: meta = child | feature << 24 | default_left << 30   (bit 31 clear); child = index of the LEFT
                      child's record in `nodes` (forest-global, 24 bits), the right child is child + 1
       leaf:          meta = 1 << 31 | ordinal; ordinal = forest-global leaf number (trees in order; within a tree
                      its root first, then its other records in order)
     leaf_values: n_leaves values by ordinal, f32 (XGBoost) or f64 (both sklearn kinds); info->leaf_bytes is 4 or 8
     leaf_ids:    n_leaves original node ids by ordinal (xgboost pred_leaf / sklearn apply)
   A tree whose root is a leaf, and a degenerate chain, are valid. Limits (FD_ERR_UNSUPPORTED, named in the message):
   at most 2^24 nodes in the forest (the child field), num_feature <= 64 (the feature field; also the LDS tile).
   FD_ERR_INVALID_ARG: a child index outside its tree, a node reached twice (a cycle or a shared subtree).
   Call with NULL buffers to query sizes in *info; capacities are counted in records / values / ids. */
typedef struct {
  int32_t kind;
  int32_t n_trees;
  int32_t depth;      /* deepest leaf over all trees (a root leaf has depth 0) */
  int32_t leaf_bytes; /* 4 or 8 */
  int64_t n_nodes;
  int64_t n_leaves;
  float base_margin;  /* XGB: f32 margin seeded by base_score */
  int32_t pad;
} fd_sparse_info;
int fd_pack_forest_sparse_host(const fd_forest_params* params, const fd_tree_arrays* trees, void* nodes,
                               int64_t nodes_cap, void* leaf_values, int64_t values_cap, int32_t* leaf_ids,
                               int64_t ids_cap, fd_sparse_info* info);

/* ---------------------------------------------------------------- forest attribution (TreeSHAP) */
/* Path-dependent TreeSHAP (Lundberg et al. 2018) of a loaded forest's RAW output: the XGBoost margin, the
   IsolationForest path-length sum, the predict_proba kind's sum of leaf fractions (what fd_forest_predict_* reports
   as raw). phi[r, f] for f < num_feature is feature f's contribution to row r's raw output, phi[r, num_feature] the
   bias (the sum over trees of the cover-weighted mean leaf value; XGBoost: plus the f32 base margin, widened), and a
   row's num_feature + 1 values sum to its raw output. All arithmetic is f64; a split is decided exactly as the walk
   decides it (f32, go left <=> x < t with sklearn's (double)x <= thr rewritten; a NaN and a column >= ld take the
   default direction).

   Covers: a split sends cover[child] / cover[node] of the weight to each child. fd_load_forest carries none;
   fd_forest_set_cover attaches one f64 per node (XGBoost sum_hessian, sklearn weighted_n_node_samples; n_nodes must be
   the forest's node count) to the forest in `slot`. Every node reachable from a root needs a finite cover > 0
   (FD_ERR_INVALID_ARG naming tree and node otherwise). fd_load_xgboost_json keeps the file's sum_hessian itself when
   every reachable node has a usable one. An explain call on a slot without covers fails with FD_ERR_NOT_LOADED. */
#define FD_SHAP_MAX_PATH 16 /* unique features on one root-to-leaf path */
#define FD_SHAP_MAX_TOPK 16
int fd_forest_set_cover(fd_engine* eng, int slot, const double* cover, int64_t n_nodes);
/* Host-only: the sum_hessian arrays of an XGBoost JSON file, concatenated in fd_xgboost_json_read's node order.
   cover == NULL: only *n_nodes. FD_ERR_INVALID_ARG when a tree has no sum_hessian or cap is too small. */
int fd_xgboost_json_read_cover(const char* path, double* cover, int64_t cap, int64_t* n_nodes);

/* Host-only: the path table the kernel streams. One record per leaf, trees in order, a tree's leaves in left-first
   depth-first order. A path's elements are the UNIQUE features on it in order of first appearance; repeated splits on
   a feature are merged: the row must lie in [lo, hi) (lo = -inf without a lower bound; has_hi = 0 and hi = +inf
   without an upper one), nan_follows = every such edge is its node's default direction, z = the product of the edges'
   cover ratios. pz = the product of a path's z (the share of the training weight that reaches the leaf). A tree whose
   root is a leaf gives one path of length 0. A path with more than FD_SHAP_MAX_PATH unique features:
   FD_ERR_UNSUPPORTED naming the tree. Call with NULL buffers for the sizes in *info. */
typedef struct {
  int64_t elem_offset; /* first element in the element array */
  int32_t len;         /* unique features on the path */
  int32_t tree;
  double value;        /* leaf value (XGBoost: the f32 weight, widened) */
  double pz;
} fd_shap_path;
typedef struct {
  int32_t feature;
  float lo, hi;
  uint8_t nan_follows;
  uint8_t has_hi;
  uint8_t pad[2];
  double z;
} fd_shap_elem;
typedef struct {
  int64_t n_paths, n_elems;
  int32_t max_len;  /* longest path (unique features) */
  int32_t n_chunks; /* the kernel's fixed split of the table: chunk c holds paths [c * chunk_paths, ...) */
  int64_t chunk_paths;
  double bias;      /* sum of value * pz in path order (+ the XGBoost base margin) */
} fd_shap_info;
int fd_shap_paths_host(const fd_forest_params* params, const fd_tree_arrays* trees, const double* cover,
                       fd_shap_path* paths, int64_t paths_cap, fd_shap_elem* elems, int64_t elems_cap,
                       fd_shap_info* info);

/* Host-only reference: recursive TreeSHAP on the trees themselves (Algorithm 2 of the paper), f64, no path table.
   phi: n x ld_phi, ld_phi >= num_feature + 1; columns past num_feature are left alone. */
int fd_forest_shap_ref_host(const fd_forest_params* params, const fd_tree_arrays* trees, const double* cover,
                            const float* X, int64_t n, int32_t ld, double* phi, int32_t ld_phi);

/* The kernel. d_X: n x ld f32 as for fd_forest_predict_device. d_rows == NULL: every row is explained, phi is n x
   ld_phi (n_rows is ignored); else phi row j explains X row d_rows[j], j < n_rows — the caller of the _device variant
   guarantees 0 <= d_rows[j] < n (a row outside is written as NaN), the _host variant checks (FD_ERR_INVALID_ARG).
   ld_phi >= num_feature + 1. A row's values are a function of that row and the forest only: bit-identical whatever
   n, the row's position, d_rows or the run (per feature the table's chunks are summed path by path, then the chunk
   sums in chunk order; no atomics). The path table is built on the first call for a slot and dropped on unload /
   reload; FD_ERR_UNSUPPORTED as fd_shap_paths_host. Counter "forest_shap_launches". */
int fd_forest_shap_device(fd_engine* eng, int slot, const float* d_X, int64_t n, int32_t ld, const int64_t* d_rows,
                          int64_t n_rows, double* d_phi, int32_t ld_phi);
int fd_forest_shap_host(fd_engine* eng, int slot, const float* X, int64_t n, int32_t ld, const int64_t* rows,
                        int64_t n_rows, double* phi, int32_t ld_phi);

/* Reason codes: per row of phi (n x ld_phi f64) the k <= FD_SHAP_MAX_TOPK largest of columns 0 .. num_feature-1 (the
   bias column is not a candidate), by |phi| (by_abs != 0) or by signed phi; ties go to the lower column. A value of
   0.0 (or NaN) is never reported; unused places hold idx = -1, val = 0. idx: n x k i32, val: n x k f64 (the signed
   value). */
int fd_shap_topk_device(fd_engine* eng, const double* d_phi, int64_t n, int32_t ld_phi, int32_t num_feature, int32_t k,
                        int32_t by_abs, int32_t* d_idx, double* d_val);
int fd_shap_topk_host(fd_engine* eng, const double* phi, int64_t n, int32_t ld_phi, int32_t num_feature, int32_t k,
                      int32_t by_abs, int32_t* idx, double* val);

/* ---------------------------------------------------------------- training: histogram GBDT (ModelTrainer) */
/* Replaces ModelTrainer.train_xgboost_model's fit (ml/training/model_trainer.py:83-96): a depth-wise histogram
   gradient-boosting fit of a binary:logistic gbtree forest, whose result is an fd_tree_arrays forest that
   fd_load_forest serves and an XGBoost JSON file can carry. The arithmetic is the engine's own and declared (DESIGN
   §4.14, csrc/gbdt_row.h); it is not XGBoost's bit for bit (no weighted quantile sketch, fixed-point gradients, a
   counter-based sample). The device path (_device / _host) and the single-threaded reference (_ref_host) compile the
   same rule header and return the same bits.

   Cuts: per feature the sorted non-NaN column v (n_f values); candidates v[floor(k n_f / max_bin)], k = 1 ..
   max_bin - 1, made unique, a candidate equal to v[0] dropped, at most 254 kept (the lowest). bin(x) = #{cuts <= x},
   NaN -> bin 255; a row goes left at cut j iff x < cut_j iff bin(x) <= j.
   Gradients: p = sigma(margin) by a deterministic f64 sigmoid (no exp()), g = p - y and h = p (1 - p) rounded to
   nearest-even multiples of 2^-24 (int32; h at least one quantum); every sum is int64, so a histogram is the same
   bits for any grid and any arrival order.
   Sample: row i is in round t's sample iff fmix64(seed ^ mix(t, i)) < subsample * 2^64; colsample_bytree keeps the
   max(1, floor(c F)) features with the smallest fmix64(seed ^ mix(t, f)), ties to the lower index. Rows outside the
   sample enter no histogram but are routed and receive the leaf's margin update.
   Split: per node, kept feature and cut j two candidates (missing right, missing left), gain = GL^2/(HL+lambda) +
   GR^2/(HR+lambda) - G^2/(H+lambda) in f64 from the exactly converted sums; valid iff HL, HR >= min_child_weight;
   the best under (gain desc, feature asc, cut asc, missing-right first); split iff gain > 1e-6 and depth < max_depth.
   Leaf: w = (float)(-G / (H + lambda) * eta); margins add w in f32 in tree order (as fd_forest_predict_*). */
typedef struct {
  int32_t n_rounds;  /* trees, 1 .. 65536 */
  int32_t max_depth; /* 1 .. 10 */
  int32_t max_bin;   /* 2 .. 256 */
  int32_t reserved;
  double eta;
  double lambda;           /* >= 0 */
  double min_child_weight; /* >= 0; lambda + min_child_weight > 0 */
  double subsample;        /* (0, 1] */
  double colsample_bytree; /* (0, 1] */
  double base_score;       /* (0, 1): the margin starts at the loader's -logf(1 / base_score - 1) */
  uint64_t seed;
} fd_gbdt_params;

/* A grown forest in caller arrays: the fd_tree_arrays members (trees->... are written despite their const, as by
   fd_xgboost_json_read; nodes in XGBoost's breadth-first depth-wise numbering, threshold = the cut's f32 value,
   leaf_value = the f32 leaf weight, both widened) and per node sum_hessian (the node's H), loss_changes (the chosen
   gain, 0 at leaves) and base_weights (-G / (H + lambda) * eta at every node). */
typedef struct {
  fd_tree_arrays* trees;
  double* sum_hessian;
  double* loss_changes;
  double* base_weights;
} fd_gbdt_model;

/* Host-only. X: n x ld f32, F <= 64 model columns. cuts == NULL or offsets == NULL: only *n_cuts (the total).
   Else offsets[F + 1] and cuts[*n_cuts]: feature f's cuts are cuts[offsets[f] .. offsets[f + 1]), ascending. */
int fd_gbdt_cuts_host(const float* X, int64_t n, int32_t ld, int32_t F, int32_t max_bin, float* cuts,
                      int32_t* offsets, int64_t* n_cuts);
/* The u8 matrix, n x F row-major. _device: device pointers, on the engine's stream; _host: host pointers through the
   kernel; _ref_host: plain C++. */
int fd_gbdt_bin_device(fd_engine* eng, const float* d_X, int64_t n, int32_t ld, int32_t F, const float* d_cuts,
                       const int32_t* d_offsets, uint8_t* d_bins);
int fd_gbdt_bin_host(fd_engine* eng, const float* X, int64_t n, int32_t ld, int32_t F, const float* cuts,
                     const int32_t* offsets, uint8_t* bins);
int fd_gbdt_bin_ref_host(const float* X, int64_t n, int32_t ld, int32_t F, const float* cuts, const int32_t* offsets,
                         uint8_t* bins);
/* margins (f32) and labels (0 / 1) -> the fixed-point pairs; _host runs the kernel, _ref_host plain C++ */
int fd_gbdt_grad_host(fd_engine* eng, const float* margin, const uint8_t* y, int64_t n, int32_t* g, int32_t* h);
int fd_gbdt_grad_ref_host(const float* margin, const uint8_t* y, int64_t n, int32_t* g, int32_t* h);
/* One tree from a binned matrix (n x F), int32 (g, h), a row mask (NULL: every row) and a feature mask (bit f of
   feature_mask: feature f is searched): the integer-in, tree-out seam of the split search. Of params only max_depth,
   eta, lambda and min_child_weight are read. out's arrays hold 2^(max_depth + 1) - 1 nodes and trees->tree_offsets
   two entries; *n_nodes receives the tree's size. _device: d_bins, d_g, d_h, d_row_mask are device pointers, the
   cuts and the outputs host pointers (the call waits for the engine's stream). */
int fd_gbdt_grow_tree_device(fd_engine* eng, const uint8_t* d_bins, int64_t n, int32_t F, const float* cuts,
                             const int32_t* offsets, const int32_t* d_g, const int32_t* d_h, const uint8_t* d_row_mask,
                             uint64_t feature_mask, const fd_gbdt_params* params, fd_gbdt_model* out, int64_t* n_nodes);
int fd_gbdt_grow_tree_host(fd_engine* eng, const uint8_t* bins, int64_t n, int32_t F, const float* cuts,
                           const int32_t* offsets, const int32_t* g, const int32_t* h, const uint8_t* row_mask,
                           uint64_t feature_mask, const fd_gbdt_params* params, fd_gbdt_model* out, int64_t* n_nodes);
int fd_gbdt_grow_tree_ref_host(const uint8_t* bins, int64_t n, int32_t F, const float* cuts, const int32_t* offsets,
                               const int32_t* g, const int32_t* h, const uint8_t* row_mask, uint64_t feature_mask,
                               const fd_gbdt_params* params, fd_gbdt_model* out, int64_t* n_nodes);
/* The fit: X n x ld f32 (F <= min(ld, 64) model columns), y n labels (0 / 1), n <= 2^28 (FD_ERR_UNSUPPORTED above).
   Two calls, as fd_xgboost_json_read: with out == NULL *n_nodes receives the node capacity to allocate (n_rounds *
   (2^(max_depth + 1) - 1)) and nothing runs; with out (arrays of that capacity, tree_offsets n_rounds + 1) the forest
   is grown and *n_nodes receives its size. margins (n f32, may be NULL): the final margins, exactly what
   fd_forest_predict_* reports as raw for the rows of X under the returned forest. _device: d_X, d_y and d_margins
   are device pointers, out host arrays. The fit loop issues launches only: no copy or wait per level or tree; the
   trees come back in one copy at the end. FD_ERR_INVALID_ARG: F outside 1..64, max_bin outside 2..256, max_depth
   outside 1..10, a label other than 0 / 1 (_host and _ref_host check; _device trusts the caller), subsample or
   colsample_bytree outside (0, 1], the other limits of fd_gbdt_params. Counters "gbdt_hist_launches", "gbdt_trees",
   "gbdt_nodes_split". Option "gbdt_hist_rows": rows per workgroup of the histogram kernel (results identical). */
int fd_gbdt_fit_device(fd_engine* eng, const float* d_X, const uint8_t* d_y, int64_t n, int32_t ld, int32_t F,
                       const fd_gbdt_params* params, fd_gbdt_model* out, int64_t* n_nodes, float* d_margins);
int fd_gbdt_fit_host(fd_engine* eng, const float* X, const uint8_t* y, int64_t n, int32_t ld, int32_t F,
                     const fd_gbdt_params* params, fd_gbdt_model* out, int64_t* n_nodes, float* margins);
int fd_gbdt_fit_ref_host(const float* X, const uint8_t* y, int64_t n, int32_t ld, int32_t F,
                         const fd_gbdt_params* params, fd_gbdt_model* out, int64_t* n_nodes, float* margins);

/* The fit watched on a held-out set (XGBClassifier.fit(..., eval_set=[(X_test, y_test)]), model_trainer.py:83-96),
   with early stopping and a class weight. Rules (csrc/gbdt_row.h, DESIGN §4.14 "Evaluation"):
   Class weight: with scale_pos_weight = w a positive row's g = quantise(w (p - 1)), h = max(1, quantise(w p (1 - p)));
   negative rows are unchanged; w == 1 gives the bits of fd_gbdt_fit_*. 0 < w <= 64 (FD_ERR_INVALID_ARG) and
   n max(1, w) <= 2^28 (FD_ERR_UNSUPPORTED above). Evaluation is not weighted.
   Eval margins: the eval matrix is binned with the training cuts; after round t every eval row adds tree t's leaf to
   its f32 margin (from the base margin, in tree order: what fd_forest_predict_* reports as raw).
   AUC: key(m) is a u32 ordered like the f32 margin, -0 and +0 equal, every NaN one key above +inf's. With P / N the
   eval set's positives / negatives, 2U = sum over positive rows of #{negatives with key < its key} + #{negatives with
   key <= its key}; auc = (double)(2U) / (double)(2 P N). Error: #{rows with (margin > 0) != y} / n. Both are an
   integer count and one division: the bits do not depend on the launch shape.
   Stopping (early_stopping_rounds = k > 0): round t improves iff its metric is strictly better (AUC: greater, error:
   less) than the best so far, round 0 always; after k consecutive rounds without improvement the fit stops:
   rounds_run = best_iteration + k + 1, else n_rounds. Every grown tree is returned (rounds_run trees: tree_offsets[0
   .. rounds_run] are written): truncating to best_iteration + 1 trees is the caller's choice. */
#define FD_GBDT_METRIC_AUC 0
#define FD_GBDT_METRIC_ERROR 1
typedef struct {
  /* in */
  const float* X;    /* n x ld f32 eval rows (ld >= F); NULL or n == 0: no eval set, only the class weight acts */
  const uint8_t* y;  /* n labels, 0 / 1 */
  int64_t n;
  int32_t ld;
  int32_t metric;                /* FD_GBDT_METRIC_* */
  int32_t early_stopping_rounds; /* 0: none; > 0 needs an eval set */
  int32_t reserved;
  double scale_pos_weight; /* (0, 64] */
  /* out (each may be NULL) */
  double* metric_out;  /* n_rounds: the first rounds_run entries are written (always host memory) */
  float* margins;      /* n: the eval margins after the last round that ran */
  float* best_margins; /* the fit's n rows: the training margins after tree best_iteration */
  int32_t rounds_run;
  int32_t best_iteration; /* -1 without an eval set */
} fd_gbdt_eval;

/* As fd_gbdt_fit_* (the same two calls; eval is not read by the first), watched as `eval` says. _device: eval->X, y,
   margins and best_margins are device pointers too. The loop still issues launches only: per round the eval walk, for
   AUC a radix sort, a scan and a count, and a one-thread kernel that writes metric_out[t] and applies the stopping
   rule to a state on the device; once it stops, the fit's own kernels of later rounds return at once, and the curve,
   rounds_run and best_iteration come back in the one copy at the end. FD_ERR_INVALID_ARG: early stopping without an
   eval set; eval->ld < F; an unknown metric; for AUC an eval set of one class ("Only one class present in y_true. ROC
   AUC score is not defined in that case."; _host and _ref_host check, _device trusts its caller). Counters
   "gbdt_eval_launches", "gbdt_rounds_run"; "gbdt_trees" and "gbdt_hist_launches" advance by the rounds that ran. */
int fd_gbdt_fit_eval_device(fd_engine* eng, const float* d_X, const uint8_t* d_y, int64_t n, int32_t ld, int32_t F,
                            const fd_gbdt_params* params, fd_gbdt_eval* eval, fd_gbdt_model* out, int64_t* n_nodes,
                            float* d_margins);
int fd_gbdt_fit_eval_host(fd_engine* eng, const float* X, const uint8_t* y, int64_t n, int32_t ld, int32_t F,
                          const fd_gbdt_params* params, fd_gbdt_eval* eval, fd_gbdt_model* out, int64_t* n_nodes,
                          float* margins);
int fd_gbdt_fit_eval_ref_host(const float* X, const uint8_t* y, int64_t n, int32_t ld, int32_t F,
                              const fd_gbdt_params* params, fd_gbdt_eval* eval, fd_gbdt_model* out, int64_t* n_nodes,
                              float* margins);
/* The metric of caller margins (n f32) and labels: the sort and count path of the fit on its own. _host runs the
   kernels, _ref_host plain C++. FD_ERR_INVALID_ARG: n < 1, a label other than 0 / 1, one class only for AUC. */
int fd_gbdt_metric_host(fd_engine* eng, const float* margins, const uint8_t* y, int64_t n, int32_t metric,
                        double* out);
int fd_gbdt_metric_ref_host(const float* margins, const uint8_t* y, int64_t n, int32_t metric, double* out);
/* fd_gbdt_grad_ref_host under the class weight: the pairs the watched fit's rounds compute (plain C++) */
int fd_gbdt_grad_weighted_ref_host(const float* margin, const uint8_t* y, int64_t n, double scale_pos_weight,
                                   int32_t* g, int32_t* h);

/* ---------------------------------------------------------------- training: IsolationForest (ModelTrainer) */
/* Replaces ModelTrainer.train_isolation_forest's fit (ml/training/model_trainer.py:235-276): grows the trees of a
   scikit-learn IsolationForest (ExtraTreeRegressor(splitter="random", max_features=1) on max_samples rows drawn
   without replacement) and places offset_ at the contamination percentile of the fit rows' scores. The result is an
   fd_tree_arrays forest of kind FD_FOREST_SKLEARN_IFOREST that fd_load_forest serves. The arithmetic is the engine's
   own and declared (csrc/iforest_fit_row.h); it follows scikit-learn's algorithm wherever that is
   deterministic and replaces its Mersenne Twister stream by counter-based hashes, so the trees are not scikit-learn's
   bit for bit. The device path (_device / _host) and the single-threaded reference (_ref_host) compile the same rule
   header and return the same bits.

   psi = max_samples == 0 ? min(256, n) : min(max_samples, n); D = ceil(log2(max(psi, 2))) (at most 10).
   key = fmix64(seed + 0x9e3779b97f4a7c15); hash(t, a, tag) = fmix64(key ^ (t << 32 | a << 2 | tag)).
   Sample: tree t's j-th row (j < psi) is perm_t(j): x = j, then x = feistel_t(x) until x < n, where feistel_t is a
   4-round Feistel network on 2 b bits (b = ceil(ceil(log2 n) / 2), at least 1): (L, R) = (x >> b, x & (2^b - 1)),
   per round r (L, R) = (R, L ^ (fmix64(hash(t, r, 3) ^ R) & (2^b - 1))), result L << b | R. A bijection of [0, n):
   a tree's rows are distinct. max_features < 1 keeps the max(1, floor(max_features F)) features with the smallest
   hash(t, f, 2), ties to the lower index.
   Split: a node with m samples at depth d (heap index i, the root 0, children 2 i + 1 and 2 i + 2) is a leaf iff
   m <= 1 or d == D or no kept feature has max > min over its samples (-0 == +0; a NaN enters neither). Otherwise, of
   the c non-constant kept features in index order the r-th is split, r = (hash(t, i, 0) * c) >> 64; with mn, mx its
   min and max widened to f64 and u = (hash(t, i, 1) >> 11) * 2^-53, thr = mn + u * (mx - mn) (two roundings, no
   fma), and thr = mn unless thr < mx. A row goes left iff (double)x <= thr; default_left = 0 (a NaN goes right).
   Leaf: leaf_value = ((d + 1) + c(m)) - 1, the term the scikit-learn loader builds; c(0) = c(1) = 0, c(2) = 1,
   c(m) = 2 (ln(m - 1) + 0.5772156649015329) - 2 (m - 1) / m, one host table per fit. Nodes are numbered breadth-first
   (a split node's children take the next two numbers); n_node_samples is the node's sample count.
   if_denominator = n_estimators * c(psi). if_offset: -0.5 when contamination == 0; else the rows of X are scored with
   the grown forest (raw = the f64 sum of the leaf values in tree order, what fd_forest_predict_* reports), the sums
   sorted, and with pos = contamination (n - 1), k = floor(pos), g = pos - k, a = -2^(-raw[k] / denominator),
   b = -2^(-raw[min(k + 1, n - 1)] / denominator): offset = g < 0.5 ? a + (b - a) g : b - (b - a) (1 - g), numpy's
   linear percentile of score_samples. */
typedef struct {
  int32_t n_estimators; /* 1 .. 65536 */
  int32_t max_samples;  /* 0: min(256, n); else 2 .. 1024, clamped to n */
  double max_features;  /* (0, 1] */
  double contamination; /* 0: "auto" (offset -0.5); else (0, 0.5] */
  uint64_t seed;
} fd_iforest_fit_params;

/* The fit: X n x ld f32 (F <= min(ld, 64) model columns), 2 <= n <= 2^31 - 1 (FD_ERR_UNSUPPORTED above). Two calls, as
   fd_gbdt_fit_*: with out == NULL *n_nodes receives the node capacity n_estimators * (2^(D + 1) - 1) and nothing runs;
   with out (arrays of that capacity, tree_offsets n_estimators + 1; written despite their const) and n_node_samples
   (that capacity, may be NULL) the forest is grown, *n_nodes receives its size and *forest its kind, num_feature,
   if_offset and if_denominator. _device: d_X is a device pointer, the outputs host arrays; one workgroup grows one
   tree, all trees come back in one copy, the offset's scoring and radix sort run on the device and two f64 come back.
   FD_ERR_INVALID_ARG: n < 2, F outside 1..64, ld < F, a parameter outside its range, a non-finite value in X (_host
   and _ref_host check; _device trusts the caller and still terminates). Counters "iforest_fit_trees",
   "iforest_fit_nodes_split". */
int fd_iforest_fit_device(fd_engine* eng, const float* d_X, int64_t n, int32_t ld, int32_t F,
                          const fd_iforest_fit_params* params, fd_tree_arrays* out, double* n_node_samples,
                          fd_forest_params* forest, int64_t* n_nodes);
int fd_iforest_fit_host(fd_engine* eng, const float* X, int64_t n, int32_t ld, int32_t F,
                        const fd_iforest_fit_params* params, fd_tree_arrays* out, double* n_node_samples,
                        fd_forest_params* forest, int64_t* n_nodes);
int fd_iforest_fit_ref_host(const float* X, int64_t n, int32_t ld, int32_t F, const fd_iforest_fit_params* params,
                            fd_tree_arrays* out, double* n_node_samples, fd_forest_params* forest, int64_t* n_nodes);
/* Tree `tree`'s row ids perm_t(0 .. psi - 1) of a fit over n rows: rows holds 1024 entries, *psi receives the count.
   _host computes them in a kernel, _ref_host in plain C++. Of params max_samples and seed are read. */
int fd_iforest_fit_sample_host(fd_engine* eng, int64_t n, const fd_iforest_fit_params* params, int32_t tree,
                               int32_t* rows, int32_t* psi);
int fd_iforest_fit_sample_ref_host(int64_t n, const fd_iforest_fit_params* params, int32_t tree, int32_t* rows,
                                   int32_t* psi);
/* One tree from explicit row ids (m of them, 1 .. 1024, each in [0, n), need not be distinct; psi = m) and a feature
   mask (bit f: feature f is kept), as tree `tree` of seed params->seed: the rows-in, tree-out seam of the split rule.
   out's arrays hold 2^(D + 1) - 1 nodes and tree_offsets two entries; *n_nodes receives the tree's size. */
int fd_iforest_fit_grow_tree_host(fd_engine* eng, const float* X, int64_t n, int32_t ld, int32_t F,
                                  const int32_t* rows, int32_t m, uint64_t feature_mask,
                                  const fd_iforest_fit_params* params, int32_t tree, fd_tree_arrays* out,
                                  double* n_node_samples, int64_t* n_nodes);
int fd_iforest_fit_grow_tree_ref_host(const float* X, int64_t n, int32_t ld, int32_t F, const int32_t* rows,
                                      int32_t m, uint64_t feature_mask, const fd_iforest_fit_params* params,
                                      int32_t tree, fd_tree_arrays* out, double* n_node_samples, int64_t* n_nodes);

/* ---------------------------------------------------------------- blend (a11-a13) */
/* Replaces _calculate_model_confidence + _combine_predictions + _make_decision +
   _calculate_risk_level (ml/models/ensemble_predictor.py:252-369) for a batch.
   d_probs[m] (host array of device pointers) is model m's probability column; present[m] == 0
   drops model m as a failed prediction is dropped (:175-181). */
int fd_blend_device(fd_engine* eng, const fd_blend_params* params, int64_t n,
                    const double* const* d_probs, const uint8_t* present,
                    double* d_fraud_prob, double* d_confidence, uint8_t* d_decision, uint8_t* d_risk);
int fd_blend_host(fd_engine* eng, const fd_blend_params* params, int64_t n,
                  const double* const* probs, const uint8_t* present,
                  double* fraud_prob, double* confidence, uint8_t* decision, uint8_t* risk);

/* ---------------------------------------------------------------- card state + features (a2-a7) */
/* HBM-resident keyed state replacing the Redis round trips of the feature half:
   velocity hashes velocity:{user}:{5min|1hour|24hour} (fl/services/RedisService.java:178-207,
   fl/sinks/RedisTransactionSink.java:116-135) and the user-profile lookups (RedisService.java:83-100).
   Cards are keyed by a u64 (hash of the reference's user_id); open addressing, insert on first use. */
enum fd_window_mode {
  FD_WINDOW_REDIS_COMPAT = 0, /* session counter, TTL 3600 s refreshed per write: the reference's behaviour */
  FD_WINDOW_SLIDING = 1       /* true (t-W, t] windows over the card's last ring_k events */
};
#define FD_RAW_FEATURES 16  /* bridged Flink features per txn (column order: DESIGN.md "Features") */
#define FD_VECTOR_WIDTH 64  /* EnsemblePredictor._prepare_features width (ml/models/ensemble_predictor.py:241) */
#define FD_MAX_SEQ_LEN 16
typedef struct {
  int64_t capacity;    /* card slots (rounded up to a power of two; keep >= 2x the cards expected) */
  int32_t window_mode; /* enum fd_window_mode */
  int32_t ring_k;      /* events kept per card in sliding mode (1..64) */
  int32_t seq_len;     /* events of per-card history kept for the LSTM head (0 = off, <= 16;
                          lstm_sequential sequence_length = 10, ml/utils/config.py:152) */
} fd_state_params;
int fd_state_init(fd_engine* eng, const fd_state_params* params);
int fd_state_clear(fd_engine* eng);
int fd_state_info(fd_engine* eng, int64_t* capacity, int64_t* cards);
/* user profiles (simulator.py:40-58 UserProfile; FeatureExtractor.java:216-252, 301-313) */
typedef struct {
  int64_t n;
  const uint64_t* key;
  const double* avg_amount;        /* NaN = null (-> 0.0, FeatureExtractor.java:239-240) */
  const int32_t* account_age_days;
  const uint64_t* device_fp;       /* n x 3 fingerprint hashes, 0 = none */
} fd_users;
int fd_state_load_users_host(fd_engine* eng, const fd_users* users);
/* merchant table, replicated (simulator.py:60-75; FeatureExtractor.java:257-296) */
typedef struct {
  int64_t n;
  const double* fraud_rate;      /* NaN = null (-> 0.05) */
  const double* risk_multiplier; /* MerchantProfile.getRiskMultiplier() (class absent in the reference) */
} fd_merchants;
int fd_load_merchants_host(fd_engine* eng, const fd_merchants* merchants);
/* one micro-batch of transactions in arrival order (SoA; device pointers for _device, host for _host) */
typedef struct {
  const uint64_t* card_key;
  const int64_t* ts_ms;
  const int64_t* amount_cents;
  const int32_t* merchant;   /* index into the merchant table, -1 = unknown */
  const uint64_t* device_fp; /* 0 = null */
  const uint8_t* ip_class;   /* 0 = null, 1 = private, 2 = public (FeatureExtractor.java:434-445) */
  const uint8_t* hour;       /* Transaction.hourOfDay, 255 = null (-> UTC hour of ts) */
  const uint8_t* weekend;    /* Transaction.isWeekend, 255 = null (-> ISO day >= 6) */
} fd_txn_batch;
/* Replaces FeatureExtractor.extractAllFeatures + the velocity read/write + FeatureProcessor +
   _prepare_features for a batch: per card in arrival order, read-before-write. Outputs the scoring
   vectors (n x 64 f32) and optionally the bridged raw features (n x FD_RAW_FEATURES f64). */
int fd_features_device(fd_engine* eng, const fd_txn_batch* txns, int64_t n, float* d_vectors, double* d_raw);
int fd_features_host(fd_engine* eng, const fd_txn_batch* txns, int64_t n, float* vectors, double* raw);

/* ---------------------------------------------------------------- full feature map + rule scores (a3, (f)) */
/* FeatureExtractor.extractAllFeatures as a whole (fl/features/FeatureExtractor.java:50-493): the 64
   features of FeatureStore.getRegisteredFeatures (fl/features/FeatureStore.java:325-365, that order),
   f64, NaN where the Java map would have no key; string features as the host's vocabulary codes
   (FD_CODE_UNKNOWN for the literal "unknown"). Plus the Flink rule scores that consume them:
   FeatureEnrichmentProcessor (calculateFeatureBasedFraudScore, combine with the incoming score,
   updateRiskLevel; fl/processors/FeatureEnrichmentProcessor.java:80-93,122-367) and TransactionProcessor
   (calculateBasicFeatures, applyFraudDetectionRules, makeFinalDecision with minimal profiles for
   unknown users / merchants; fl/processors/TransactionProcessor.java:143-508). */
#define FD_FEATURE_MAP_WIDTH 64
#define FD_CODE_UNKNOWN 254
/* per-transaction context beyond fd_txn_batch; any pointer may be NULL (= all null) */
typedef struct {
  const double* geo_lat;          /* Transaction.geolocation lat / lon, NaN = absent */
  const double* geo_lon;
  const double* merchant_lat;     /* Transaction.merchantLocation lat / lon, NaN = absent */
  const double* merchant_lon;
  const uint8_t* payment_method;  /* vocabulary code, 255 = null */
  const uint8_t* transaction_type;
  const uint8_t* card_type;
  const uint8_t* user_agent_flag; /* analyzeSuspiciousUserAgent (host-side string test), 255 = null UA */
  const double* fraud_score;      /* incoming Transaction.fraudScore, NaN = null */
} fd_txn_context;
typedef struct {
  double tp_score;      /* TransactionProcessor fraud score */
  double fe_score;      /* FeatureEnrichmentProcessor fraud score */
  uint8_t tp_decision;  /* enum fd_decision */
  uint8_t tp_risk;      /* enum fd_risk */
  uint8_t fe_decision;
  uint8_t fe_risk;
  uint8_t pad[4];
} fd_rule_scores;
/* UserProfile fields beyond fd_users (simulator.py:40-58); keyed like fd_users; NULL arrays = null */
typedef struct {
  int64_t n;
  const uint64_t* key;
  const double* risk_score;        /* NaN = null */
  const uint8_t* kyc_status;       /* vocabulary code, 255 = null */
  const uint8_t* verified;         /* UserProfile.isVerified() */
  const int8_t* pref_start;        /* preferred hours, -1 = null */
  const int8_t* pref_end;
  const double* weekend_activity;  /* behavioral pattern values, NaN = absent */
  const double* online_preference;
  const double* intl_preference;   /* international_transactions, NaN = null */
  const int32_t* txn_frequency;    /* -1 = null */
  const uint8_t* has_patterns;     /* getBehavioralPatterns() != null */
} fd_users_ext;
/* MerchantProfile fields beyond fd_merchants (simulator.py:60-75), indexed like fd_merchants */
typedef struct {
  int64_t n;
  const double* avg_amount;           /* NaN = null */
  const uint8_t* risk_level;          /* 0 low, 1 medium, 2 high (vocabulary), 255 = null */
  const uint8_t* blacklisted;         /* 255 = null */
  const uint8_t* category;            /* vocabulary code, 255 = null */
  const uint8_t* high_risk_category;  /* MerchantProfile.isHighRiskCategory() */
  const uint8_t* open_hour;           /* operating hours [open, close), 255 = null */
  const uint8_t* close_hour;
  const uint8_t* suspicious_name;     /* analyzeMerchantName (host regexes), 255 = null name */
} fd_merchants_ext;
int fd_state_load_users_ext_host(fd_engine* eng, const fd_users_ext* users);
int fd_load_merchants_ext_host(fd_engine* eng, const fd_merchants_ext* merchants);
/* 256 flags each: payment-method code -> isHighRiskPaymentMethod, transaction-type code -> "refund" */
int fd_load_vocab_host(fd_engine* eng, const uint8_t* payment_high_risk, const uint8_t* type_is_refund);
/* fd_features_* plus the feature map (n x FD_FEATURE_MAP_WIDTH f64) and rule scores; d_fmap / d_rules /
   d_raw may be NULL. Advances the card state exactly like fd_features_device. */
int fd_features_full_device(fd_engine* eng, const fd_txn_batch* txns, const fd_txn_context* ctx, int64_t n,
                            float* d_vectors, double* d_raw, double* d_fmap, fd_rule_scores* d_rules);

/* ---------------------------------------------------------------- LSTM sequence head (a10) */
/* Replaces _load_tensorflow_model / _predict_tensorflow (ml/models/model_manager.py:162-165, 313-319)
   for lstm_sequential (ml/utils/config.py:145-157). Model: 1-layer LSTM(hidden = 128) over a sequence
   of per-event inputs (input_size <= 16), gates in Keras / PyTorch order i, f, g, o, then a dense head:
   n_out = 1 -> sigmoid(z), n_out = 2 -> softmax(z)[1] (_predict_tensorflow takes [:, 1] when the output
   has 2 columns, else flattens). Weights in PyTorch layout, f32 (the host converts Keras kernels):
   w_ih [4H x input_size], w_hh [4H x H], b_ih / b_hh [4H] (either may be NULL), w_out [n_out x H],
   b_out [n_out]. Computed in f32 on the matrix cores. */
typedef struct {
  int32_t input_size;
  int32_t hidden;
  int32_t n_out;
  const float* w_ih;
  const float* w_hh;
  const float* b_ih;
  const float* b_hh;
  const float* w_out;
  const float* b_out;
} fd_lstm_params;
int fd_load_lstm(fd_engine* eng, const fd_lstm_params* params);
int fd_unload_lstm(fd_engine* eng);
/* d_seq: n x T x 16 f32 (events oldest -> newest, inputs beyond input_size ignored); d_prob: n f64 */
int fd_lstm_predict_device(fd_engine* eng, const float* d_seq, int64_t n, int32_t T, double* d_prob);
int fd_lstm_predict_host(fd_engine* eng, const float* seq, int64_t n, int32_t T, double* prob);
/* In fd_score_batch_device / fd_score_records_device, a model whose slot is FD_SLOT_LSTM is the LSTM head
   over each transaction's card history (the last seq_len events including itself, fd_state_params.seq_len
   > 0); it runs on a second stream concurrently with the forests. fd_features_seq_device also returns
   those sequences (n x seq_len x 16 f32). */
#define FD_SLOT_LSTM 64
int fd_features_seq_device(fd_engine* eng, const fd_txn_batch* txns, int64_t n, float* d_vectors, double* d_raw,
                           float* d_seq);

/* ---------------------------------------------------------------- PyTorch MLP head (graph_neural) */
/* Replaces _create_pytorch_model_architecture (ml/models/model_manager.py:202-242) for the registry's
   model_type "pytorch" entry graph_neural: n_layers nn.Linear layers (defaults 64 -> 64 -> 64 -> 2), ReLU after
   every layer but the last (torch.relu: a NaN stays a NaN), dropout the identity in eval(), softmax(dim=1).
   Weights in PyTorch layout, f32: layer i's weight [dims[i+1] x dims[i]] row-major (nn.Linear.weight), its bias
   [dims[i+1]] or NULL (zeros). Non-finite weights are accepted and computed. Computed in f32 on the matrix cores.
   Limits (FD_ERR_UNSUPPORTED, named in the message): n_layers in [2, 8]; in_dim = dims[0] in [1, 64]; every hidden
   width in [1, 64]; dims[n_layers] == 2 (the reference always builds output_dim = 2). FD_ERR_INVALID_ARG: a NULL
   weight, a nonzero dims entry beyond dims[n_layers]. */
typedef struct {
  int32_t n_layers;                 /* Linear layers, 2..8 */
  int32_t dims[9];                  /* dims[0] = in_dim, dims[i+1] = layer i's outputs; dims[n_layers] == 2 */
  const float* weight[8];           /* layer i: [dims[i+1] x dims[i]] row-major (PyTorch nn.Linear.weight) */
  const float* bias[8];             /* layer i: [dims[i+1]] or NULL */
} fd_mlp_params;
/* Replaces _load_pytorch_model (ml/models/model_manager.py:168-179: torch.load + load_state_dict). One MLP per
   engine; a load replaces the previous one. Validates and packs with fd_pack_mlp_host. */
int fd_load_mlp(fd_engine* eng, const fd_mlp_params* params);
/* The reference drops a model by deleting its registry entry (reload_model, :348-369; cleanup, :405-414); idempotent. */
int fd_unload_mlp(fd_engine* eng);
/* The loaded model's shape (get_model_info's metadata, :393-399): layer count, dims[0], dims[1]; any may be NULL.
   FD_ERR_NOT_LOADED without a model. */
int fd_mlp_info(fd_engine* eng, int32_t* n_layers, int32_t* in_dim, int32_t* hidden);
/* Replaces _predict_pytorch (ml/models/model_manager.py:321-330): d_prob[i] = softmax(model(X[i]))[1], the f32
   value widened to f64. X: n rows of ld-strided f32, ld >= in_dim (FD_ERR_INVALID_ARG otherwise); columns >= in_dim
   are never read. FD_ERR_NOT_LOADED without a model; n == 0 does nothing. */
int fd_mlp_predict_device(fd_engine* eng, const float* d_X, int64_t n, int32_t ld, double* d_prob);
int fd_mlp_predict_host(fd_engine* eng, const float* X, int64_t n, int32_t ld, double* prob);
/* Every load-time check and the packing of fd_load_mlp, without a device (_create_pytorch_model_architecture's
   shape rules, :202-242): writes the packed model (header, then per layer the weights in the kernel's operand order
   and the padded bias) to blob when it is not NULL (FD_ERR_INVALID_ARG when cap is too small) and its size to
   *bytes. */
int fd_pack_mlp_host(const fd_mlp_params* params, void* blob, int64_t cap, int64_t* bytes);
/* In the scoring calls (fd_score_matrix_*, fd_score_batch_*, fd_score_records_*, fd_sharded_step) a model whose
   slot is FD_SLOT_MLP is the MLP over the batch's scoring vectors (the ensemble's graph_neural member,
   ml/models/ensemble_predictor.py's per-model predict over the same features). */
#define FD_SLOT_MLP 65

/* ---------------------------------------------------------------- training: the PyTorch MLP member (ModelTrainer) */
/* Fits the MLP that fd_load_mlp serves (the registry's graph_neural entry; the reference's trainer promises such a
   trainer and holds none). The semantics are the engine's own and declared (csrc/mlp_fit_row.h):
   minibatch training of n_layers nn.Linear layers, ReLU and inverted dropout (scale 1 / (1 - dropout)) after every
   layer but the last, loss = cross_entropy(logits, y, weight = [1, pos_weight]) with mean reduction (the weighted sum
   over the batch's rows divided by the sum of their weights), optimiser torch.optim.Adam (bias correction, weight_decay
   as L2 added to the gradient) or torch.optim.SGD (momentum, weight_decay, no Nesterov, no dampening), state in f32.
   key = fmix64(seed + 0x9e3779b97f4a7c15). Epoch e's row order is the stable ascending sort of the rows r by
   fmix64(key ^ (e << 32 | r)); step j of an epoch takes rows [j batch_size, min(n, (j + 1) batch_size)) of that order
   (the last batch is the short remainder, its mean over its own rows). Global step s = e ceil(n / batch_size) + j.
   Unit u of hidden layer i of the batch's row b (its position in the batch) is kept at step s iff
   fmix64(fmix64(~key ^ (s << 3 | i)) ^ (b << 6 | u)) >> 32 >= floor(dropout 2^32).
   A batch's gradient is the sum of per-chunk partials, a chunk being one 16-row tile of the batch (rows 16 c .. 16 c +
   15 of the batch): each partial is an f32 sum over the chunk's rows, the partials are added in ascending chunk order
   in an f64 accumulator, divided there by the batch's weight sum and rounded to f32 once. No float atomics,
   and the bits of a fit depend on neither the grid nor the option "mlp_fit_chunks_per_wg". Each step's loss is reduced
   the same way and accumulated per epoch in f64; loss_curve[e] is the mean of epoch e's batch losses. The optimiser's
   scalars (1 - beta1, 1 - beta2, lr / (1 - beta1^t), sqrt(1 - beta2^t)) are formed in f64 and rounded to f32, as
   torch hands them to its f32 tensor operations.
   Limits as fd_pack_mlp_host's (FD_ERR_UNSUPPORTED: n_layers outside 2..8, a width outside 1..64, outputs != 2);
   FD_ERR_INVALID_ARG: epochs < 1, batch_size < 1, n < 1, ld < dims[0], dropout outside [0, 1), pos_weight or a
   constant of the optimiser not finite or out of its range, a null initial weight; FD_ERR_UNSUPPORTED:
   batch_size > 65536, n > 2^31 - 1, epochs * n > 2^29 (the index arrays of every epoch are built once). The initial
   weights are the caller's (fdengine.mlp.random_weights gives nn.Linear's default ranges; a fitted model warm-starts). */
#define FD_MLP_OPT_ADAM 0
#define FD_MLP_OPT_SGD 1
typedef struct {
  int32_t n_layers;               /* 2..8 */
  int32_t dims[9];                /* as fd_mlp_params */
  int32_t epochs;                 /* >= 1 */
  int32_t batch_size;             /* 1..65536 */
  int32_t optimizer;              /* FD_MLP_OPT_* */
  int32_t reserved;
  double lr, beta1, beta2, eps;   /* Adam: lr > 0, betas in [0, 1), eps > 0; SGD reads lr */
  double momentum;                /* SGD, [0, 1) */
  double weight_decay;            /* >= 0 */
  double dropout;                 /* [0, 1) */
  double pos_weight;              /* > 0: the weight of a row of class 1 */
  uint64_t seed;
  const float* init_weight[8];    /* layer i: [dims[i+1] x dims[i]] row-major */
  const float* init_bias[8];      /* layer i: [dims[i+1]] or NULL (zeros) */
} fd_mlp_fit_params;
/* Host arrays the fit (or fd_mlp_grad_*: the gradients) is written to: weight[i] [dims[i+1] x dims[i]], bias[i]
   [dims[i+1]], loss_curve [epochs] (fd_mlp_grad_*: one value, the batch's loss; may be NULL), steps (optimiser steps
   run; fd_mlp_grad_*: 0). */
typedef struct {
  float* weight[8];
  float* bias[8];
  double* loss_curve;
  int64_t steps;
} fd_mlp_fit_out;
/* The whole fit. X n x ld f32 (columns >= dims[0] are never read), y n bytes of 0 / 1. _device: d_X and d_y are device
   pointers; _host stages them once. The fit is a stream of two launches per step (mlp_fit_step_kernel: forward,
   backward and the chunk partials on v_mfma_f32_16x16x4_f32; mlp_fit_update_kernel: the ordered sum, the optimiser,
   the operand blobs rewritten in place) with no copy or wait between steps; weights and loss_curve come back once.
   _host and _ref_host refuse (FD_ERR_INVALID_ARG) a label outside {0, 1} and a non-finite value in X; _device trusts the
   caller (any nonzero label counts as 1). _ref_host: the same rules in single-threaded plain C++, no device; it sums
   in its own order, so it agrees with the device to rounding, not bit for bit. Counters "mlp_fit_steps",
   "mlp_fit_launches" (2 per step; fd_mlp_grad_*: 2 per call). */
int fd_mlp_fit_device(fd_engine* eng, const float* d_X, const uint8_t* d_y, int64_t n, int32_t ld,
                      const fd_mlp_fit_params* params, fd_mlp_fit_out* out);
int fd_mlp_fit_host(fd_engine* eng, const float* X, const uint8_t* y, int64_t n, int32_t ld,
                    const fd_mlp_fit_params* params, fd_mlp_fit_out* out);
int fd_mlp_fit_ref_host(const float* X, const uint8_t* y, int64_t n, int32_t ld, const fd_mlp_fit_params* params,
                        fd_mlp_fit_out* out);
/* Loss and every gradient of ONE batch (the n rows of X in their order, 1 <= n <= 65536) at the weights params->init_*:
   what a step computes before its optimiser. masks: NULL (every unit kept), or (n_layers - 1) x n x 64 bytes, nonzero =
   kept, [layer][row][unit]; a kept unit is scaled by 1 / (1 - params->dropout). Of params the shape, dropout, pos_weight
   and the weights are read. _device: d_X, d_y, d_masks are device pointers, out host arrays. */
int fd_mlp_grad_device(fd_engine* eng, const float* d_X, const uint8_t* d_y, int64_t n, int32_t ld,
                       const fd_mlp_fit_params* params, const uint8_t* d_masks, fd_mlp_fit_out* out);
int fd_mlp_grad_host(fd_engine* eng, const float* X, const uint8_t* y, int64_t n, int32_t ld,
                     const fd_mlp_fit_params* params, const uint8_t* masks, fd_mlp_fit_out* out);
int fd_mlp_grad_ref_host(const float* X, const uint8_t* y, int64_t n, int32_t ld, const fd_mlp_fit_params* params,
                         const uint8_t* masks, fd_mlp_fit_out* out);
/* What a fit of n rows trains on: order (n entries, may be NULL) receives epoch `epoch`'s row order, masks (may be
   NULL; (n_layers - 1) x rows x 64 bytes, the layout fd_mlp_grad_* reads) the dropout masks of global step `step`,
   *rows that step's batch rows. Of params the shape, epochs, batch_size, dropout and seed are read. _host: plain C++.
   _device: the order as the fit uploads it, read back from the device; the masks by a kernel of the step kernel's
   hash. */
int fd_mlp_fit_batch_host(int64_t n, const fd_mlp_fit_params* params, int32_t epoch, int64_t step, int32_t* order,
                          uint8_t* masks, int32_t* rows);
int fd_mlp_fit_batch_device(fd_engine* eng, int64_t n, const fd_mlp_fit_params* params, int32_t epoch, int64_t step,
                            int32_t* order, uint8_t* masks, int32_t* rows);

/* ---------------------------------------------------------------- transaction-network features (graph detector) */
/* Replaces GraphFraudDetector._add_transaction_to_history + _calculate_network_features
   (ml/models/graph_neural_network.py:228-242, 338-392): a rolling log of recent transactions, one global arrival
   sequence per engine, and five features per transaction derived from it. Inputs are fd_txn_batch's card_key
   (0 = null user_id), merchant (-1 = null merchant_id) and amount_cents, rows in arrival order. Transaction g
   (0-based since fd_graph_init / fd_graph_clear) sees the entries [s(g), g], itself included, where with
   H = max_history, keep = ceil(H/2), P = H - keep: s(g) = 0 for g < H, else H + floor((g-H)/P)*P - keep (the
   reference cuts a full history to its newer half before appending). Later rows of a call see earlier ones; the
   results do not depend on how the stream is cut into calls. Output row: FD_GRAPH_FEATURES f64 in the order
   user_centrality, merchant_centrality, clustering_coefficient, path_length_anomaly, community_anomaly; all 0.0 for
   a row with a null user or merchant (the row still enters the log). Four columns are the reference's values;
   path_length_anomaly sums the window's amounts exactly in cents where the reference sums floats (differs by less
   than 1e-11 for positive amounts). network_risk_score (the reference runs its model over torch.randn node
   features) is not computed. The log is not part of fd_state_snapshot, and is per engine: a sharded deployment
   keeps one log per rank. */
#define FD_GRAPH_FEATURES 5
typedef struct {
  int32_t max_history; /* the reference's max_history_size (default 10000); 2..65536 */
} fd_graph_params;
/* (re)initialises an empty log; FD_ERR_INVALID_ARG for a max_history outside 2..65536 */
int fd_graph_init(fd_engine* eng, const fd_graph_params* params);
/* empties the log: the next transaction is g = 0 again. FD_ERR_NOT_LOADED before fd_graph_init (as the calls below) */
int fd_graph_clear(fd_engine* eng);
/* total: transactions since init / clear; held: the reference's transaction_history_size, g_last - s(g_last) + 1 */
int fd_graph_info(fd_engine* eng, int64_t* total, int64_t* held);
/* Appends n transactions and writes their n x FD_GRAPH_FEATURES rows. _device: device pointers, enqueued on the
   engine stream, nothing read back. n == 0 does nothing. */
int fd_graph_step_device(fd_engine* eng, const fd_txn_batch* txns, int64_t n, double* d_out);
int fd_graph_step_host(fd_engine* eng, const fd_txn_batch* txns, int64_t n, double* out);
/* The same features for a whole stream from g = 0, on the host alone (no device, no engine): the declared rule by
   direct scans of each window, with the kernels' epilogue. */
int fd_graph_features_host(const uint64_t* card_key, const int32_t* merchant, const int64_t* amount_cents, int64_t n,
                           int32_t max_history, double* out);

/* ---------------------------------------------------------------- text patterns and features (text analyzer) */
/* Replaces BertTextAnalyzer.detect_fraud_patterns and get_text_features (ml/models/bert_text_analyzer.py:283-399).
   A row is four UTF-8 fields in the fixed order merchant_name (m), description (d), category (c), location (l); a
   missing key is the empty field. The rows of a call are one byte blob and 4n + 1 offsets into it.
   Domain: rows whose four fields are all ASCII (every byte < 0x80). Any other row gets status FD_TEXT_NONASCII and
   all its outputs are 0 (exactness there needs Unicode tables: str.lower(), \d as category Nd, Unicode whitespace);
   fdengine.text.BertTextAnalyzer recomputes such rows on the host by the reference's rule.
   Byte classes (ASCII): space = 0x09-0x0D, 0x1C-0x1F, 0x20 (Python's \s and str.split()); digit = 0-9; alpha = a-z,
   A-Z; special = everything else, 0x00-0x08, 0x0E-0x1B and 0x7F included (a NUL is an ordinary byte: fields are
   delimited by offsets).
   Features, FD_TEXT_FEATURES f64 per row in the reference's dict order: merchant_name_length, description_length,
   total_text_length, merchant_name_unique_chars (distinct byte values of m after folding A-Z onto a-z),
   merchant_name_char_diversity (unique / length as one f64 division; both 0 for an empty m), numbers_in_merchant,
   numbers_in_description, total_numbers, special_chars_merchant, special_chars_description, total_special_chars,
   merchant_word_count (maximal runs of non-space bytes), description_word_count, total_word_count.
   Patterns, one byte per row: bit 0 crypto_keywords, 1 gift_card_keywords, 2 urgent_language, 3 suspicious_merchant,
   4 known_scam_patterns; a bit is set when any keyword of its list (csrc/text_row.h, 45 in all) is a substring of
   m ' ' d ' ' c ' ' l with A-Z folded onto a-z: all three separators always present, no word boundaries, a keyword
   may span fields, a space inside a keyword is 0x20 only.
   A field is shorter than 2^32 bytes. analyze_transaction_text (a model fetched by name, random logits without it)
   is not computed. */
#define FD_TEXT_FIELDS 4
#define FD_TEXT_PATTERNS 5
#define FD_TEXT_FEATURES 14
#define FD_TEXT_NONASCII 1
typedef struct {
  const uint8_t* bytes;
  const int64_t* off; /* 4n + 1 entries, off[0] = 0, non-decreasing; row i, field j occupies
                         [off[4i+j], off[4i+j+1]) of bytes */
} fd_text_batch;
/* n x FD_TEXT_FEATURES features, n pattern bytes, n status bytes; any output may be NULL; n == 0 does nothing.
   _device: device pointers, enqueued on the engine stream, nothing read back (the offsets are not checked).
   _host: host pointers; FD_ERR_INVALID_ARG for a nonzero off[0] or decreasing offsets. */
int fd_text_features_device(fd_engine* eng, const fd_text_batch* d, int64_t n, double* d_feat, uint8_t* d_patterns,
                            uint8_t* d_status);
int fd_text_features_host(fd_engine* eng, const fd_text_batch* t, int64_t n, double* feat, uint8_t* patterns,
                          uint8_t* status);
/* The same on the host alone (no device, no engine): the declared rule by direct scans, each keyword searched for in
   the joined text. */
int fd_text_features_ref_host(const uint8_t* bytes, const int64_t* off, int64_t n, double* feat, uint8_t* patterns,
                              uint8_t* status);

/* ---------------------------------------------------------------- batched scoring */
/* Replaces the per-transaction loop of /batch-predict (ml/main.py:235-249) for prepared scoring
   vectors: every forest model scores the same X, then the blend runs, all on the device.
   Model m (blend order) is either a loaded forest (slots[m] >= 0) or an externally computed
   probability column ext_probs[m] (slots[m] < 0; host pointer for _host, device for _device);
   present[m] == 0 drops model m. d_model_probs (optional) receives the n x n_models column-major
   per-model probabilities (model m at offset m*n). */
int fd_score_matrix_device(fd_engine* eng, const fd_blend_params* params, const int32_t* slots,
                           const double* const* ext_probs, const uint8_t* present, const float* d_X,
                           int64_t n, int32_t ld, double* d_model_probs, double* d_fraud_prob,
                           double* d_confidence, uint8_t* d_decision, uint8_t* d_risk);
int fd_score_matrix_host(fd_engine* eng, const fd_blend_params* params, const int32_t* slots,
                         const double* const* ext_probs, const uint8_t* present, const float* X, int64_t n,
                         int32_t ld, double* model_probs, double* fraud_prob, double* confidence,
                         uint8_t* decision, uint8_t* risk);

/* ---------------------------------------------------------------- A/B tests (assign, route, record) */
/* Replaces ABTestManager (ml/testing/ab_testing.py): a user is assigned to control (0) or treatment (1), a batch is
   scored with the model set of each row's variant, and one result per transaction is reduced per variant on the
   device. An engine holds FD_AB_MAX_TESTS tests, ids 0..7.
   Assignment: bucket = fmix64((key ? key : 1) ^ salt) % 100 with murmur3's fmix64, salt = fd_hash64(test name);
   treatment when (double)bucket < threshold, threshold being the f64 product traffic_split * 100 formed by the
   caller (0.07 * 100 is 7.000000000000001: 8 buckets, as in the reference's comparison :126). The reference's own
   hash() of a str is salted per process, so its assignments cannot be, and are not, reproduced; what holds is its
   contract: one variant per (test, user), and the treatment share of the 100 buckets.
   Recording: a row is variant (0 / nonzero), prediction, decision (enum fd_decision; another code is in no class),
   processing_time_ms and a label (0, 1, FD_AB_NO_LABEL = the reference's None). DECLINE and REVIEW are "flagged",
   APPROVE and APPROVE_WITH_MONITORING "passed" (:254, :278-285). Per variant: integer counts, and for the two float
   columns their sum and M2 = sum (x - mean)^2, each as a pair hi + lo (csrc/abtest_row.h). The list the reference's
   `precision` metric takes its moments from (:382-388) is 1.0 / 0.0 per flagged row of a variant whose rows are all
   labeled: tp + fp values, tp of them 1.0. The counts are exact; the moments depend on how a stream is cut into
   calls only in their last bits, and the same calls on the same state give the same bits every time (no float
   atomics). Not part of fd_state_snapshot; one state per engine, fd_ab_state_merge_host joins the ranks' states. */
#define FD_AB_MAX_TESTS 8
#define FD_AB_NO_LABEL 255
typedef struct {
  uint64_t salt;
  double threshold; /* traffic_split * 100, in [0, 100] */
} fd_ab_params;
typedef struct {
  double sum_hi, sum_lo; /* sum x = sum_hi + sum_lo */
  double m2_hi, m2_lo;   /* sum (x - mean)^2 = m2_hi + m2_lo */
} fd_ab_moments;
typedef struct {
  int64_t rows;
  int64_t decisions[4]; /* by enum fd_decision */
  int64_t labeled, tp, fp, tn, fn;
  fd_ab_moments prediction, time_ms; /* over all `rows` */
} fd_ab_variant_state;
typedef struct {
  fd_ab_variant_state variant[2]; /* control, treatment */
} fd_ab_state;
/* One variant's arguments of fd_score_matrix_* */
typedef struct {
  const fd_blend_params* params;
  const int32_t* slots;
  const double* const* ext_probs; /* n-long columns in arrival order (host for _host, device for _device) */
  const uint8_t* present;
} fd_ab_model_set;
/* create: an empty test (FD_ERR_INVALID_ARG for an id in use or a threshold outside [0, 100]); destroy frees the id;
   clear empties its state. FD_ERR_NOT_LOADED for an id that was not created (as in every call below). */
int fd_ab_create(fd_engine* eng, int32_t test_id, const fd_ab_params* params);
int fd_ab_destroy(fd_engine* eng, int32_t test_id);
int fd_ab_clear(fd_engine* eng, int32_t test_id);
/* n keys -> n variant bytes. _device: device pointers, enqueued on the engine stream, nothing read back. */
int fd_ab_assign_device(fd_engine* eng, int32_t test_id, const uint64_t* d_keys, int64_t n, uint8_t* d_variant);
int fd_ab_assign_host(fd_engine* eng, int32_t test_id, const uint64_t* keys, int64_t n, uint8_t* variant);
/* Stable partition of the row indices 0..n-1 by a variant column: idx holds the control rows in arrival order, then
   the treatment rows in arrival order; counts = {control, treatment}. n < 2^31. */
int fd_ab_partition_device(fd_engine* eng, const uint8_t* d_variant, int64_t n, int32_t* d_idx, int64_t* d_counts);
int fd_ab_partition_host(fd_engine* eng, const uint8_t* variant, int64_t n, int32_t* idx, int64_t* counts);
/* fd_score_matrix_* with one model set per variant: rows are assigned by key, gathered into partition order, each
   variant's rows scored by fd_score_matrix's own path for that many rows and those models, and the results put back
   in arrival order. A variant without rows launches nothing. variant (optional) receives the assignment.
   model_probs (optional) is max(n_models) x n column-major: model m of a row's own set at m*n + row, NaN where that
   set has fewer models. Waits once for the engine stream (the two counts size the launches). */
int fd_ab_score_matrix_device(fd_engine* eng, int32_t test_id, const fd_ab_model_set* control,
                              const fd_ab_model_set* treatment, const float* d_X, const uint64_t* d_keys, int64_t n,
                              int32_t ld, uint8_t* d_variant, double* d_model_probs, double* d_fraud_prob,
                              double* d_confidence, uint8_t* d_decision, uint8_t* d_risk);
int fd_ab_score_matrix_host(fd_engine* eng, int32_t test_id, const fd_ab_model_set* control,
                            const fd_ab_model_set* treatment, const float* X, const uint64_t* keys, int64_t n,
                            int32_t ld, uint8_t* variant, double* model_probs, double* fraud_prob, double* confidence,
                            uint8_t* decision, uint8_t* risk);
/* n results into the test's state. processing_time_ms: an n-long column, or NULL and time_scalar applies to every
   row (a batch caller has one time per batch). actual_fraud NULL: no row is labeled. Neither form waits for the
   kernel. _host: columns in pageable memory have been read when the call returns; columns in pinned (page-locked)
   memory are read asynchronously and must not change or be freed before fd_engine_sync or fd_ab_state_host. */
int fd_ab_record_device(fd_engine* eng, int32_t test_id, const uint8_t* d_variant, const double* d_prediction,
                        const uint8_t* d_decision, const double* d_processing_time_ms, double time_scalar,
                        const uint8_t* d_actual_fraud, int64_t n);
int fd_ab_record_host(fd_engine* eng, int32_t test_id, const uint8_t* variant, const double* prediction,
                      const uint8_t* decision, const double* processing_time_ms, double time_scalar,
                      const uint8_t* actual_fraud, int64_t n);
/* the test's state (waits for the engine stream) */
int fd_ab_state_host(fd_engine* eng, int32_t test_id, fd_ab_state* out);
/* No device, no engine. merge: out = a then b (out may be a or b). bucket: the 0..99 bucket of each key.
   record_ref: the rows in order into *state (zero it first for a new one), by the functions the kernel's lanes use. */
int fd_ab_state_merge_host(const fd_ab_state* a, const fd_ab_state* b, fd_ab_state* out);
int fd_ab_bucket_host(const uint64_t* keys, int64_t n, uint64_t salt, uint8_t* bucket_out);
int fd_ab_record_ref_host(const uint8_t* variant, const double* prediction, const uint8_t* decision,
                          const double* processing_time_ms, double time_scalar, const uint8_t* actual_fraud, int64_t n,
                          fd_ab_state* state);

/* ---------------------------------------------------------------- prediction metrics (MetricsCollector) */
/* Replaces MetricsCollector (ml/monitoring/metrics.py:30-431, called once per scored transaction by ml/main.py): the
   counters, Prometheus series and "last hour / last minute" figures of record_prediction, reduced on the device from
   the columns a scoring call leaves there. One collector per engine; not part of fd_state_snapshot.
   A row is fraud_prob p (f64), decision (enum fd_decision; another code is counted in the totals and under no
   decision), processing_time_ms (a column, or one scalar for the batch) and, per model m < n_models, model m's own
   probability model_probs[m * n + row] (NaN: the row has no such model; the layout fd_ab_score_matrix_* writes).
   Every compare is an f64 compare against the reference's literal; a histogram bucket is the first bound with
   value <= bound, the duration value being the f64 quotient processing_time_ms / 1000.0.
   Windows. A record call carries one timestamp (seconds, f64) for all its rows. The state holds a ring of `slots`
   time slots, each one timestamp and the window accumulators of the rows recorded under it: a call whose timestamp
   equals the newest slot's merges into it, a greater one opens the next slot (evicting the oldest when the ring is
   full; the summary counts evictions), a smaller one is FD_ERR_INVALID_ARG. A query at `now` reduces, oldest to
   newest, the slots with now - ts <= 3600.0 (hour) and <= 60.0 (minute), the reference's predicates (:233, :247).
   Counts are integer adds and exact. Float sums are pairs hi + lo kept by error-free additions, reduced in an order
   fixed by n and the calls alone: the same calls on the same state give the same bits (no float atomics), and
   fd_metrics_record_ref_host reduces in the kernel's order, so host and device agree to the bit call for call. */
#define FD_METRICS_MAX_MODELS 8
#define FD_METRICS_SERIES (FD_METRICS_MAX_MODELS + 1) /* "ensemble", then model 0..7 */
#define FD_METRICS_SCORE_BUCKETS 12 /* le 0.0, 0.1, ..., 1.0, +Inf (:95) */
#define FD_METRICS_TIME_BUCKETS 12  /* le 0.001, 0.005, 0.01, 0.025, 0.05, 0.1, 0.25, 0.5, 1.0, 2.5, 5.0, +Inf (:89) */
#define FD_METRICS_RISK_LEVELS 5    /* enum fd_risk */
typedef struct {
  int32_t n_models; /* 0..FD_METRICS_MAX_MODELS: the most model columns a record call may carry */
  int32_t slots;    /* ring size, 1..65536 */
} fd_metrics_params;
typedef struct {
  double hi, lo; /* the sum is hi + lo */
} fd_metrics_sum;
/* One model_name label of ml_predictions_total / ml_prediction_duration_seconds (:168-176), cumulative */
typedef struct {
  int64_t rows;                               /* duration histogram _count; model_performance[..]["predictions"] :163 */
  int64_t decisions[4];                       /* ml_predictions_total{model_name, decision}, by enum fd_decision */
  int64_t time_hist[FD_METRICS_TIME_BUCKETS]; /* per bucket, not cumulated: processing_time_ms / 1000.0 :169, :176 */
  fd_metrics_sum time_ms;                     /* model_performance[..]["total_time_ms"] :164 */
  fd_metrics_sum seconds;                     /* duration histogram _sum: the sum of the quotients */
  double last_timestamp;                      /* model_performance[..]["last_prediction"] :165; 0 without rows */
} fd_metrics_series;
typedef struct {
  int64_t predictions;                          /* prediction_count :153 */
  int64_t fraud_detections;                     /* p > 0.5 :155 */
  int64_t declined;                             /* decision == DECLINE :158 */
  int64_t score_hist[FD_METRICS_SCORE_BUCKETS]; /* ml_fraud_score_distribution per bucket, not cumulated :170 */
  int64_t risk_detected[FD_METRICS_RISK_LEVELS]; /* ml_fraud_detected_total{risk_level}: p > 0.5 only :178-181, levels :310-321 */
  fd_metrics_sum score_sum;                     /* ml_fraud_score_distribution _sum */
  fd_metrics_series series[FD_METRICS_SERIES];  /* [0] "ensemble", [1 + m] model m */
} fd_metrics_cumulative;
/* One model over a window (get_model_performance_report :337-364), over the window's rows that carry the model */
typedef struct {
  int64_t rows;               /* total_predictions :354 */
  int64_t dist[3];            /* low_risk p < 0.3, medium_risk 0.3 <= p < 0.7, high_risk p >= 0.7 :360-362 */
  fd_metrics_sum time_ms;     /* avg_processing_time_ms = sum / rows :355 */
  fd_metrics_sum prediction;  /* avg_prediction_score = sum / rows :358 */
  double min_time_ms, max_time_ms; /* :356-357; 0 without rows */
} fd_metrics_window_model;
typedef struct {
  int64_t rows;           /* predictions_last_hour / _last_minute :287-288, :235 */
  int64_t fraud;          /* p > 0.5: fraud_detections_last_hour :256, :292 */
  int64_t high_risk;      /* p > 0.8: high_risk_transactions :293 */
  fd_metrics_sum time_ms; /* avg_processing_time_ms = sum / rows :260 */
  fd_metrics_window_model model[FD_METRICS_MAX_MODELS];
} fd_metrics_window;
typedef struct {
  fd_metrics_cumulative total;
  fd_metrics_window hour, minute; /* slots with now - ts <= 3600.0 / <= 60.0 */
  int64_t evictions;              /* slots dropped from a full ring since init / clear */
  int64_t slots_used;
  double newest;                  /* the newest slot's timestamp; 0 when none */
} fd_metrics_summary;
/* init: (re)creates an empty collector (FD_ERR_INVALID_ARG for n_models or slots out of range); clear empties it.
   FD_ERR_NOT_LOADED before fd_metrics_init (as in the calls below that take an engine). */
int fd_metrics_init(fd_engine* eng, const fd_metrics_params* params);
int fd_metrics_clear(fd_engine* eng);
/* n rows under one timestamp. _device: device pointers (the outputs of fd_score_matrix_device /
   fd_ab_score_matrix_device as they are), enqueued on the engine stream, waits for nothing. d_model_probs may be NULL
   when n_models is 0; d_time_ms NULL: time_scalar for every row. n < 2^31; n == 0 does nothing.
   _host: columns in pageable memory have been read when the call returns; columns in pinned (page-locked) memory are
   read asynchronously and must not change or be freed before fd_engine_sync or fd_metrics_query_host. */
int fd_metrics_record_device(fd_engine* eng, const double* d_fraud_prob, const uint8_t* d_decision,
                             const double* d_model_probs, int32_t n_models, const double* d_time_ms,
                             double time_scalar, double timestamp, int64_t n);
int fd_metrics_record_host(fd_engine* eng, const double* fraud_prob, const uint8_t* decision,
                           const double* model_probs, int32_t n_models, const double* time_ms, double time_scalar,
                           double timestamp, int64_t n);
/* the summary at `now` (waits for the engine stream; one struct is read back, never the ring) */
int fd_metrics_query_host(fd_engine* eng, double now, fd_metrics_summary* out);
/* No device, no engine: the same collector in caller memory of fd_metrics_state_bytes(slots) bytes (0 for slots out
   of range), by the functions the kernels' lanes use and in the kernels' order of reduction. state_init_host makes it
   empty. summary_merge_host: out = a then b (out may be a or b): counts add, sums add error-free, min / max / last
   combine; it joins the summaries of a sharded deployment's ranks taken at one `now`. */
int64_t fd_metrics_state_bytes(int32_t slots);
int fd_metrics_state_init_host(void* state, const fd_metrics_params* params);
int fd_metrics_record_ref_host(void* state, const double* fraud_prob, const uint8_t* decision,
                               const double* model_probs, int32_t n_models, const double* time_ms, double time_scalar,
                               double timestamp, int64_t n);
int fd_metrics_query_ref_host(const void* state, double now, fd_metrics_summary* out);
int fd_metrics_summary_merge_host(const fd_metrics_summary* a, const fd_metrics_summary* b, fd_metrics_summary* out);

/* The whole hot path for one micro-batch of transactions: fd_features_* (card state read/update,
   scoring vectors) then fd_score_matrix_* on those vectors (ld = FD_VECTOR_WIDTH). d_vectors may be
   NULL (engine scratch). Equivalent to the reference's per-transaction chain
   FeatureExtractor -> RedisTransactionSink -> FeatureProcessor -> EnsemblePredictor.predict. */
int fd_score_batch_device(fd_engine* eng, const fd_blend_params* params, const int32_t* slots,
                          const double* const* ext_probs, const uint8_t* present, const fd_txn_batch* txns,
                          int64_t n, float* d_vectors, double* d_model_probs, double* d_fraud_prob,
                          double* d_confidence, uint8_t* d_decision, uint8_t* d_risk);

/* Streaming form of fd_score_batch_device for a sequence of micro-batches (the Flink operator chain is
   pipelined record by record; here micro-batch by micro-batch). Same results, same card-state order.
   Batch i's feature and scoring launches run on one of the engine's two private pipeline streams
   (alternating by batch), the features ordered after batch i-1's feature launches and after
   `input_ready` (a hipEvent_t the caller recorded once the batch's input columns were in device memory;
   NULL = they were complete before this call). Batch i+1's features therefore overlap batch i's forests.
   The scoring launches write engine-owned staging; the caller's output buffers are written by one copy
   kernel queued on the ENGINE stream (fd_engine_set_stream) after batch i's scoring: the outputs are
   ordered on the engine stream exactly as with fd_score_batch_device, and a caller may free or reuse
   them in that stream's order (e.g. torch's caching allocator on the stream the engine is bound to).
   d_vectors (optional, n x FD_VECTOR_WIDTH f32) receives the batch's scoring vectors the same way.
   The input columns must stay unchanged until the engine stream has passed the call (the engine stream
   waits for the batch's features and scoring). Any other engine call in between orders the next
   batch's features after everything queued on the engine stream (no overlap across it). */
int fd_score_batch_pipelined(fd_engine* eng, const fd_blend_params* params, const int32_t* slots,
                             const double* const* ext_probs, const uint8_t* present, const fd_txn_batch* txns,
                             int64_t n, float* d_vectors, double* d_model_probs, double* d_fraud_prob,
                             double* d_confidence, uint8_t* d_decision, uint8_t* d_risk, void* input_ready);

/* per-transaction window / sink inputs beyond fd_txn_batch; any pointer may be NULL */
typedef struct fd_window_inputs_s {
  const uint8_t* payment_method; /* vocabulary code, 255 = null (NULL: all null) */
  const uint8_t* is_fraud;       /* Transaction.isFraud, nonzero = TRUE (NULL: all false) */
  const double* fraud_score;     /* Transaction.fraudScore, NaN = null (NULL: all null) */
} fd_window_inputs;

/* ---------------------------------------------------------------- card-hash sharding */
/* The reference partitions per-card work by key (Kafka key / Flink keyBy(userId),
   fl/FraudDetectionJob.java; velocity state in one Redis, fl/services/RedisService.java:178-207).
   Here GPU r of G owns the cards with fd_shard_of(card_key, G) == r and keeps their state in its HBM.
   One micro-batch step on G GPUs (the host shim drives the two RCCL all-to-alls):
     ingest GPU : fd_route_partition_device   -> records grouped by owner (stable) + per-owner counts
     (all-to-all of counts, then of FD_ROUTE_RECORD_BYTES records)
     owner GPU  : fd_score_records_device      -> features + forests + blend, FD_RESULT_RECORD_BYTES records
     (all-to-all of result records back, reversed splits)
     ingest GPU : fd_route_scatter_results_device -> results in the micro-batch's original order.
   Records from one source keep their arrival order, so every card sees its transactions in
   (step, ingest rank, ingest index) order. */
#define FD_MAX_SHARDS 64
#define FD_ROUTE_RECORD_BYTES 48
#define FD_RESULT_RECORD_BYTES 24
/* owner shard of each key (host-only; what the shim uses to load each GPU's user profiles) */
int fd_shard_of_host(const uint64_t* keys, int64_t n, int32_t n_shards, int32_t* out);
/* d_records: n x FD_ROUTE_RECORD_BYTES, owner-major, stable; d_counts: n_shards int64 (device) */
int fd_route_partition_device(fd_engine* eng, const fd_txn_batch* txns, int64_t n, int32_t n_shards,
                              void* d_records, int64_t* d_counts);
/* same, the records also carrying the window / sink inputs the owner needs (extra may be NULL; its
   payment_method and is_fraud are read, fraud_score is produced by the owner) */
int fd_route_partition_ex_device(fd_engine* eng, const fd_txn_batch* txns, const fd_window_inputs* extra,
                                 int64_t n, int32_t n_shards, void* d_records, int64_t* d_counts);
/* the same on the caller's `stream` (a hipStream_t; its own scratch), leaving the engine stream and the
   pipelined stream undisturbed: the pipelined sharded step partitions the next micro-batch and exchanges its
   counts while the owner GPUs still score the current one (fdengine/sharding.py) */
int fd_route_partition_stream(fd_engine* eng, const fd_txn_batch* txns, const fd_window_inputs* extra,
                              int64_t n, int32_t n_shards, void* d_records, int64_t* d_counts, void* stream);
/* owner side: received records (+ their result records, may be NULL) back to columns for the window /
   sink kernels: out's non-NULL fields (card_key, ts_ms, amount_cents, merchant, device_fp, ip_class, hour,
   weekend) and payment_method / is_fraud / fraud_score (the result's fraud_prob; NaN without results) */
int fd_route_unpack_device(fd_engine* eng, const void* d_records, const void* d_results, int64_t n,
                           const fd_txn_batch* out, uint8_t* d_payment_method, uint8_t* d_is_fraud,
                           double* d_fraud_score);
/* the whole hot path (fd_score_batch_device) over received records; d_results: n x FD_RESULT_RECORD_BYTES
   {f64 fraud_prob, f64 confidence, u32 seq, u8 decision, u8 risk, u16 pad} in the records' order */
int fd_score_records_device(fd_engine* eng, const fd_blend_params* params, const int32_t* slots,
                            const uint8_t* present, const void* d_records, int64_t n, void* d_results);
/* streaming form over received records (fd_score_batch_pipelined's pipeline: features on the engine's
   pipeline streams after the previous batch's features and after `input_ready` — the event the caller
   recorded once the records' all-to-all had landed —, scoring, then d_results written on the engine
   stream, where the caller queues the return all-to-all). The owner's batch i+1 features overlap batch i's
   forests; the records must stay unchanged until the engine stream has passed the call. */
int fd_score_records_pipelined(fd_engine* eng, const fd_blend_params* params, const int32_t* slots,
                               const uint8_t* present, const void* d_records, int64_t n, void* d_results,
                               void* input_ready);
/* The sharded step as one call over the engine's own RCCL communicators (csrc/comm.hip): the host loads
   RCCL once (the process's librccl.so, by path; any library exporting ncclGetUniqueId, ncclCommInitRank,
   ncclCommDestroy, ncclCommAbort, ncclGroupStart/End, ncclSend/Recv, ncclAllGather and ncclGetErrorString can stand in — the tests run several
   ranks on one GPU over an in-process loopback of that API), rank 0 makes two unique ids (fd_comm_unique_id), the
   host broadcasts them, every rank calls fd_comm_init (collective, blocking with RCCL). fd_sharded_step then runs
   one micro-batch: its split sizes (exchanged by the previous call when it prefetched this batch, else now: the
   step's one host wait), then, on the engine's forward stream behind the wait for this batch's inbox slot, ONE
   RCCL group holding this batch's records to their owners (ncclSend/ncclRecv with per-peer counts) and — with
   `next` (optional: prefetch) — the next batch's count exchange (from 4 ranks one ncclAllGather of every rank's
   per-peer send counts right after the group, below that 2 x world point-to-point operations inside it: engine
   option count_exchange), its
   count kernel queued before the group and its publish + places after it (so the next counts land while this
   batch is scored), then the owner's
   features + scoring (fd_score_records_pipelined's pipeline, the features waiting for the records), the
   results back (second communicator, engine stream) and into arrival order in the caller's outputs (device or
   host-mapped memory), written on the engine stream. The calling thread issues every communicator operation, in
   one fixed order; every rank makes the same calls in the same order (the same prefetch pattern).
   Batch ids (caller-chosen): `next_id` (nonzero) names the prefetched batch; the call that scores it passes the
   same id as `batch_id`. batch_id 0 means "not the prefetched batch": a pending prefetch is dropped (its count
   exchange completes, its records are never sent — every rank must drop alike). A nonzero batch_id that is not
   the pending one (or with nothing pending) fails with FD_ERR_INVALID_ARG and changes nothing. The caller keeps a prefetched batch's input
   columns alive and unchanged until the call that scores (or drops) it has returned.
   split_sizes (optional): the 2 x world send / receive counts of this batch.
   Failure: the split-size wait gives up after the engine option comm_timeout_ms (a peer that never posts its counts)
   or on a stream error; it first aborts both communicators (ncclCommAbort: RCCL's kernels blocked on the peer exit),
   then fails with FD_ERR_HIP. Later fd_sharded_step calls fail with the abort's reason; fd_engine_sync,
   fd_comm_destroy and fd_engine_destroy wait on the streams at most comm_timeout_ms each; fd_comm_destroy then
   fd_comm_init makes new communicators. */
int fd_comm_unique_id(const char* rccl_path, uint8_t* id_out /* 128 bytes */);
int fd_comm_init(fd_engine* eng, const char* rccl_path, int32_t rank, int32_t world, const uint8_t* id_fwd,
                 const uint8_t* id_back);
int fd_comm_destroy(fd_engine* eng);
int fd_sharded_step(fd_engine* eng, const fd_blend_params* params, const int32_t* slots, const uint8_t* present,
                    const fd_txn_batch* txns, int64_t n, uint64_t batch_id, void* input_ready,
                    const fd_txn_batch* next, int64_t next_n, uint64_t next_id, void* next_ready,
                    double* d_fraud_prob, double* d_confidence, uint8_t* d_decision, uint8_t* d_risk,
                    int64_t* split_sizes);
/* out[seq] = result for each of the n returned records; conf/decision/risk may be NULL.
   fd_engine_sync reports a record whose seq is outside [0, n). */
int fd_route_scatter_results_device(fd_engine* eng, const void* d_results, int64_t n, double* d_fraud_prob,
                                    double* d_confidence, uint8_t* d_decision, uint8_t* d_risk);

/* ---------------------------------------------------------------- Flink window aggregates (a5) */
/* WindowProcessor.processUserVelocity / processMerchantPatterns (fl/windows/WindowProcessor.java:36-66)
   with UserVelocityAggregateFunction (:248-352) and MerchantAggregateFunction (:357-484), evaluated per
   micro-batch on the device: keyBy(card key) sliding 5 min / slide 1 min, keyBy(merchant) tumbling 1 h,
   event time with BoundedOutOfOrderness watermarks. Micro-batch semantics (DESIGN.md "Windows"): after a
   batch's events are added, the watermark becomes max(previous, max event time - lag - 1) and every window
   whose last millisecond it passed fires once with the events of its range that arrived so far (later
   arrivals are late for it and dropped, allowed lateness 0). Transactions with an unknown merchant (-1)
   are not aggregated by merchant (keyBy on a null id). Amount sums are exact integer cents. */
typedef struct {
  int64_t log_capacity;            /* events kept per log (user / merchant), 40 B each, device-resident */
  int64_t max_out_of_orderness_ms; /* watermark lag: forBoundedOutOfOrderness(10 s) = 10000 */
} fd_window_params;

/* UserVelocityAggregate (getResult :292-311) + the Flink window bounds; 96 B */
typedef struct {
  uint64_t user_key;
  int64_t window_start, window_end; /* Flink TimeWindow [start, end) */
  int64_t first_ts, last_ts;        /* accumulator windowStart / windowEnd: min / max event time (ms) */
  int32_t count, fraud_count, high_risk_count, unique_merchants, unique_payment_methods, pad;
  double total_amount, avg_amount, fraud_rate, velocity_score;
} fd_user_window;
/* MerchantAggregate (getResult :403-424) + the Flink window bounds + the exact moments it is derived from
   (what fd_merchant_windows_merge combines across shards); 168 B */
typedef struct {
  int32_t merchant, count;
  int64_t window_start, window_end, first_ts, last_ts;
  int32_t fraud_count, high_risk_count, unique_users, unique_payment_methods;
  double total_amount, fraud_amount, avg_amount, fraud_rate, amount_stddev, risk_score;
  int64_t cents, fraud_cents;   /* exact amount sums (integer cents) */
  uint64_t sq_lo, sq_hi;        /* sum of cents^2, 128-bit */
  uint64_t pm_mask[4];          /* payment-method codes seen (bit per code) */
} fd_merchant_window;
/* allocate the event logs and reset the watermark (needs fd_state_init: cards are keyed by its table;
   fd_state_init / fd_state_clear empty the logs and reset the watermark too). After a failed step
   (FD_ERR_OOM) the window state is unspecified until the next fd_windows_init. */
int fd_windows_init(fd_engine* eng, const fd_window_params* params);
/* add one micro-batch (device pointers) and return the windows that fired, into host arrays of the given
   capacities (FD_ERR_OOM if more fired); with flush != 0 the watermark then moves past every held event
   (end of input: Flink's final MAX_WATERMARK) and all remaining windows fire. Synchronous. */
int fd_windows_step_device(fd_engine* eng, const fd_txn_batch* txns, const fd_window_inputs* in, int64_t n,
                           int flush, fd_user_window* user_out, int64_t user_cap, int64_t* n_user,
                           fd_merchant_window* merchant_out, int64_t merchant_cap, int64_t* n_merchant);
/* same, host input pointers (staged to the device) */
int fd_windows_step_host(fd_engine* eng, const fd_txn_batch* txns, const fd_window_inputs* in, int64_t n,
                         int flush, fd_user_window* user_out, int64_t user_cap, int64_t* n_user,
                         fd_merchant_window* merchant_out, int64_t merchant_cap, int64_t* n_merchant);
/* current watermark (INT64_MIN before the first) and events held in the user / merchant logs */
int fd_windows_stats(fd_engine* eng, int64_t* watermark, int64_t* user_events, int64_t* merchant_events);
/* Sharded windows: every shard advances ONE watermark — before its step, each shard reports the
   largest event time of the whole node's micro-batch (an all-reduce MAX of the ingest batches); the next step
   then advances the watermark from it even when this shard received no transaction. Each shard's user
   windows are complete (cards are owned); its merchant windows are partials over its cards. */
int fd_windows_observe(fd_engine* eng, int64_t max_event_ts);
/* Merge merchant-window partials of several shards (host memory, any order): records with the same
   (merchant, window_start) are combined from their exact moments (counts, cents, cents^2, payment-method
   set, first / last time; distinct users add: a card lives on one shard) and the derived fields recomputed
   exactly as the device does. out: capacity n; *n_out merged records sorted by (window_start, merchant).
   Host only (no GPU needed). */
int fd_merchant_windows_merge(const fd_merchant_window* parts, int64_t n, fd_merchant_window* out, int64_t* n_out);

/* ---------------------------------------------------------------- sink aggregates */
/* RedisTransactionSink.updateAggregations (fl/sinks/RedisTransactionSink.java:140-262): per transaction the
   hourly:{ts/3600000}, daily:{ts/86400000} and merchant:{merchant}:{ts/3600000} summaries (count, amount,
   fraud count, high-risk count (hourly, fraudScore > 0.7), distinct users (merchant)), HBM-resident.
   Amounts are exact integer cents (reported / 100); the reference's 30-min Redis TTL is wall-clock, so
   retention here is explicit (fd_sink_evict_before). Declared semantics: DESIGN.md §4.8. */
typedef struct {
  int64_t capacity;      /* aggregate entries (hourly + daily + merchant-hour buckets held at once) */
  int64_t user_capacity; /* distinct (merchant, hour, card) members held at once */
} fd_sink_params;
enum fd_agg_kind { FD_AGG_HOURLY = 1, FD_AGG_DAILY = 2, FD_AGG_MERCHANT = 3 };
typedef struct { /* the stored aggregation map (updateHourly/Daily/MerchantAggregations :165-262); 64 B */
  int64_t total_count, fraud_count, high_risk_count, unique_user_count;
  double total_amount, fraud_rate, avg_amount;
  int32_t found, pad;
} fd_aggregate;
int fd_sink_init(fd_engine* eng, const fd_sink_params* params);
/* apply one micro-batch (device pointers; card_key, ts_ms, amount_cents, merchant of fd_txn_batch; is_fraud /
   fraud_score of fd_window_inputs, NULL = false / null). Synchronous (error check). */
int fd_sink_update_device(fd_engine* eng, const fd_txn_batch* txns, const fd_window_inputs* in, int64_t n);
int fd_sink_update_host(fd_engine* eng, const fd_txn_batch* txns, const fd_window_inputs* in, int64_t n);
/* RedisService.getAggregation: bucket = hour or day key, merchant index for FD_AGG_MERCHANT (else ignored) */
int fd_sink_query_host(fd_engine* eng, int32_t kind, const int64_t* bucket, const int32_t* merchant, int64_t n,
                       fd_aggregate* out);
/* drop every bucket older than hour_key (a day is kept while any of its hours is) */
int fd_sink_evict_before(fd_engine* eng, int64_t hour_key, int64_t* kept_entries, int64_t* kept_users);

/* ---------------------------------------------------------------- state snapshot / restore */
/* Durable image of the HBM keyed state: the counterpart of Flink's keyed-state checkpoints
   (fl/FraudDetectionJob.java:112-136) and the Redis RDB of the velocity / profile hashes
   (config/redis/redis-master.conf:6-13). Key-addressed (one record per card: header, fingerprints, ring,
   LSTM history, extended profile), then the replicated merchant / vocabulary tables and the window event
   logs; per-section FNV-1a-64 checksums. Synchronous; written to `path`.tmp then renamed.
   (shard, n_shards) are recorded in the image for bookkeeping (0, 1 for an unsharded engine). */
int fd_state_snapshot(fd_engine* eng, const char* path, int32_t shard, int32_t n_shards, int64_t* bytes_written);
/* Re-insert an image's cards by key into the current table (any capacity; window_mode / ring_k / seq_len
   must match fd_state_init's) keeping only the cards with shard_of(key, n_shards) == shard — restoring
   every old shard's image on every new shard re-shards the state onto a different GPU count. Replicated
   tables are replaced. Window logs are appended (fd_windows_init first) unless FD_RESTORE_SKIP_WINDOWS;
   images merged onto one engine must share the window watermark. The image also carries the sink aggregates
   (replaced on restore; same shard / shard count only, else FD_RESTORE_SKIP_SINK) and the ingest codec's merchant /
   vocabulary tables (replaced). On FD_ERR_IO / FD_ERR_OOM the state is unspecified until fd_state_clear. */
#define FD_RESTORE_SKIP_WINDOWS 1
#define FD_RESTORE_SKIP_SINK 2 /* sink aggregates (fd_sink_*) resume only on the same shard / shard count */
int fd_state_restore(fd_engine* eng, const char* path, int32_t shard, int32_t n_shards, int32_t flags,
                     int64_t* cards_restored);

/* ---------------------------------------------------------------- Kafka JSON ingest codec */
/* TransactionDeserializationSchema.deserialize (fl/serialization/TransactionDeserializationSchema.java:28-49)
   of the simulator's messages (json.dumps(asdict(Transaction), default=str),
   services/data-simulator/src/main/python/simulator.py:77-101,186,376-385) on the device: one micro-batch of
   raw messages (concatenated bytes + n+1 offsets) -> the SoA columns below. Identities: card_key =
   fd_hash64(user_id), device_fp = fd_hash64(device_fingerprint), txn_hash = fd_hash64(transaction_id);
   merchant = index of merchant_id in fd_ingest_set_merchants (-1 unknown / null); payment_method /
   transaction_type / card_type = index in fd_ingest_set_vocab (255 null, FD_VOCAB_OTHER unknown);
   ip_class 0 null / 1 private / 2 public and user_agent_flag 0 / 1 / 255 null (FeatureExtractor.java:434-451);
   ts_ms = ISO-8601 timestamp as epoch ms (UTC without offset); amount_cents exact. A number counts by its first
   19 significant digits; strings and keys are decoded (JSON escapes) before they are read. Declared semantics and
   limits: DESIGN.md "Ingest". Rows with status & FD_INGEST_INVALID are the reference's ERROR placeholder
   (all other columns default). Any output pointer may be NULL. */
#define FD_VOCAB_OTHER 254
enum fd_vocab_kind { FD_VOCAB_PAYMENT_METHOD = 0, FD_VOCAB_TRANSACTION_TYPE = 1, FD_VOCAB_CARD_TYPE = 2 };
enum fd_ingest_status {
  FD_INGEST_MALFORMED = 1,     /* not one JSON object / bad member syntax / value of the wrong type */
  FD_INGEST_TOO_LONG = 2,      /* message longer than 4080 bytes */
  FD_INGEST_UNKNOWN_VOCAB = 4, /* a payment / type / card string outside its vocabulary (code FD_VOCAB_OTHER) */
  FD_INGEST_INEXACT = 8,       /* sub-cent amount (rounded half-even), an amount with a non-zero digit beyond the
                                  19th, or a double whose digits beyond the 19th could change its rounding */
  FD_INGEST_MISSING = 16,      /* user_id, amount or timestamp missing / null */
};
#define FD_INGEST_INVALID (FD_INGEST_MALFORMED | FD_INGEST_TOO_LONG | FD_INGEST_MISSING)
typedef struct {
  uint64_t* card_key;
  int64_t* ts_ms;
  int64_t* amount_cents;
  int32_t* merchant;
  uint64_t* device_fp;
  uint8_t* ip_class;
  uint8_t* hour;
  uint8_t* weekend;
  double* geo_lat;
  double* geo_lon;
  double* merchant_lat;
  double* merchant_lon;
  uint8_t* payment_method;
  uint8_t* transaction_type;
  uint8_t* card_type;
  uint8_t* user_agent_flag;
  double* fraud_score;
  uint8_t* is_fraud;
  uint64_t* txn_hash;
  uint8_t* status;
} fd_ingest_out;
/* the identity hash of the codec: fmix64(FNV-1a-64(bytes)) (host; profiles / merchants are keyed with it) */
int fd_hash64(const uint8_t* bytes, int64_t n, uint64_t* out);
/* vocabulary `which` (enum fd_vocab_kind): string i (bytes[offsets[i]..offsets[i+1])) gets code i (n <= 254) */
int fd_ingest_set_vocab(fd_engine* eng, int32_t which, const uint8_t* bytes, const int64_t* offsets, int64_t n);
/* merchant_id strings in merchant-table order (index = the engine's merchant index) */
int fd_ingest_set_merchants(fd_engine* eng, const uint8_t* bytes, const int64_t* offsets, int64_t n);
/* device pointers (HBM-resident messages, outputs); asynchronous on the engine stream; n <= 2^30 */
int fd_ingest_json_device(fd_engine* eng, const uint8_t* d_bytes, const int64_t* d_offsets, int64_t n,
                          const fd_ingest_out* d_out);
/* host pointers (staged through the device); synchronous */
int fd_ingest_json_host(fd_engine* eng, const uint8_t* bytes, const int64_t* offsets, int64_t n,
                        const fd_ingest_out* out);
/* the codec's scalar conversions on the host (diagnostics / tests): kind 0 = JSON number text -> f64
   (correctly rounded), 1 = amount text -> cents, 2 = ISO-8601 text -> epoch ms. flags: bit 0 grammar error,
   bit 1 inexact. */
int fd_ingest_scalar_host(int32_t kind, const uint8_t* text, int32_t n, double* f64_out, int64_t* i64_out,
                          int32_t* flags_out);

/* ---------------------------------------------------------------- diagnostics */
/* Per-launch device timing of the engine's hot kernels, measured with HIP events recorded on the
   launch stream around each kernel. fd_timing_read synchronises and returns the summed time (ms) and
   count of the timed launches of `kind` (FD_TIMING_ALL: every kind) since the last fd_timing_reset.
   A forest launch counts under FD_TIMING_XGB for an XGBoost forest, FD_TIMING_IFOREST for both sklearn kinds. */
enum fd_timing_kind { FD_TIMING_ALL = -1, FD_TIMING_XGB = 0, FD_TIMING_IFOREST = 1, FD_TIMING_FEATURES = 2,
                      FD_TIMING_BLEND = 3, FD_TIMING_ROUTE = 4, FD_TIMING_LSTM = 5,
                      FD_TIMING_WINDOWS = 6, FD_TIMING_INGEST = 7,
                      FD_TIMING_ENSEMBLE = 8 /* fused XGBoost + IsolationForest + blend kernel */,
                      FD_TIMING_MLP = 9 /* the MLP head's kernel (fd_mlp_predict_*, FD_SLOT_MLP) */,
                      FD_TIMING_GRAPH = 10 /* one fd_graph_step_*: every kernel of its chunks */,
                      FD_TIMING_TEXT = 11 /* one fd_text_features_*: every kernel of its chunks */,
                      FD_TIMING_ABTEST = 12 /* the A/B kernels, one entry per step: assign, partition, gather,
                                               scatter, record (the scoring passes of fd_ab_score_matrix_* count
                                               under their own kinds) */ };
int fd_engine_set_timing(fd_engine* eng, int enable);
/* Engine tuning knobs (for A/B measurement; defaults are the tuned choices):
     "forest_kernel": 0 auto, 1 force the 256-thread kernel, 2 force the 1024-thread tree-split kernel
     on the threshold layout, 3 force the 1024-thread kernel on the binned layout, 6 force the tree-split
     small-batch path (auto takes it below 128 tiles of 256 transactions), 8 force the binned node-only-chunk
     kernel (auto's choice when the forest has that layout), 11 force the sparse-layout kernel (forest_sparse_kernel:
     nodes read from global memory; its image is built on the first such launch for a forest that has the heap
     layouts). A FD_FOREST_SKLEARN_PROBA forest or one deeper than 10 levels has the sparse layout only and takes
     that kernel whatever this option says; the variants measured slower were removed (their numbers 4, 5, 7, 9
     and 10 stay refused)
     "ensemble": 1 fused XGBoost + IsolationForest + blend kernel when applicable (default), 0 per-model kernels
     "ensemble_chunks": the fused kernel's chunk layout, 0 (default) auto: compact once the engine has RCCL
     communicators (fd_comm_init), else wide; 1 wide (24 XGBoost / 16 IsolationForest trees per chunk, 148 KB of
     LDS); 2 compact (20 / 12, 132 KB: room for an RCCL kernel on the same CU). Outputs are identical.
     "ensemble_contract": the fused kernel on the pipelined stream's compact / split rows walks the forests contracted
     against the rows' constant slots (fd_contract_forest_host): 4 (default) the dense chunk stream of
     fd_dense_layout_host — trees as perfect heaps of their bundle's depth in blocks of their own size, up to 8
     bundles per chunk and barrier, the bundles dealt to the tree groups by depth — with a chunk's trees sorted by
     depth before they are cut into bundles; 3 the same with bundles of consecutive trees; 1 the padded chunks, each
     tree to the deepest of its wave's trees; 2 each tree to its own depth (slower); 0 the full forests (1, 2, 0: A/B
     options). Outputs are identical.
     "lstm_rows": LSTM tile, 0 auto (4 transactions below 4096, else 16), 4 or 16
     "mlp_form": the MLP head's kernel for the reference shape (3 layers, padded widths 64): 0 (default) weights in
     registers, 1 the LDS form every other shape takes
     "mlp_fit_chunks_per_wg": the MLP fit's step kernel, chunks (16-row tiles of the batch) a workgroup takes in turn:
       0 (default) one each, up to 2^30 (one workgroup for the whole batch); every value gives the same bits
     "mlp_wgs_per_cu": the MLP head's persistent grid, workgroups per CU: 0 (default) two where they fit, else 1..8
     (capped by what fits)
     "timing_every": N >= 1, fd_engine_set_timing records HIP events on one launch in N of each timing kind
     (the others run without event records; fd_timing_read's launch count is the timed ones)
     "small_streams": latency batches (< 32768 transactions) with the LSTM head and / or several forests: 0
     (default) all on the engine stream (no cross-queue hops; config 5 0.088 ms per 1 k step), 1 the LSTM and the
     forests after the first on one side stream (0.095), 2 on two side streams (0.095)
     "pipeline_lean": fd_score_batch_pipelined's bucket pass, 1 (default) the lean kernel that fits beside the
     fused ensemble kernel, 0 the full bucket kernel
     "pipeline_gather": fd_score_batch_pipelined's batches of <= 4096 transactions (option slot_gather on, no slot
     stream), 1 (default) the gather bucket kernel (card slots found inside it: one feature launch), 0 the slot +
     lean bucket pair of the large batches
     (The compact rows' eight small-integer slots are always binned by one lookup in a per-plan table of the bins of
     0..31; round 5's option to search them instead was removed after its A/B)
     "ensemble_bin_global": the fused kernel's compact rows, 1 every varying slot binned by a search of its merged
     threshold table in global memory (L2-resident; no staging pass, chunk 0's DMA issued at the kernel's start),
     0 (default) the tables staged in LDS first (outputs identical)
     "lean_group": how the lean bucket kernel groups a bucket's keys by card (outputs identical): 2 (default) an
     LDS hash table of card slots (no sort), 1 a rank sort split over all threads, 0 the first m threads each rank
     one key over the whole list
     "latency_prebin": latency batches scored by the XGBoost + IsolationForest pair path with the LSTM head: the
     pair's tree-split binning in the LSTM launch (no binning launch; counter "latency_prebinned_batches"), 3
     (default) inside the LSTM's own workgroups, a binary-search level per recurrence step (2 where a thread would
     take more than two searches), 2 in extra workgroups after the LSTM's own, 1 ahead of them; 0 its own binning
     launch (outputs identical)
     (further options — "slot_stream", "slot_gather", "bucket_spread", "feature_prio", "ensemble_prio",
     "compact_vectors", "latency_fused", "seq_ring_lstm", "bucket_keys" — are listed with their measurements in
     DESIGN.md §3)
     "comm_timeout_ms": fd_sharded_step's split-size wait fails with FD_ERR_HIP after this many ms (default
     120000): a peer that never posts its counts (a dead rank, a different call pattern) becomes an error, not a hang
     "count_exchange": fd_sharded_step's per-peer counts as 1 one ncclAllGather per batch, 0 2 x world
     ncclSend/ncclRecv in the records group, -1 (default) the all-gather from 4 ranks (every rank the same; not while
     a prefetched batch is pending)
     "stream_priority": HIP priorities of the engine's pipeline and forward streams (ROCm keeps a hardware-queue
     pool per priority, so they stop sharing queues with the engine stream and RCCL's streams): 0 all default, 1
     the two pipeline streams high, 2 + the forward stream low, 3 (default) + the forward stream high. Set before
     the first pipelined call and fd_comm_init. */
int fd_engine_set_option(fd_engine* eng, const char* key, int64_t value);
/* Engine counters (diagnostics): "window_saturated" (sliding windows: transactions so far whose 24 h window held the
   ring's whole capacity K of prior events — their counts may be truncated at K; synchronises the engine's streams),
   "pipelined_batches" (batches through fd_score_batch_pipelined /
   fd_score_records_pipelined so far), "pipelined_compact_batches" (of those, scored by the fused ensemble kernel from
   the compact 64-B rows: no vectors requested), "ensemble_single_launches" (fd_forest_predict batches scored by the
   fused kernel over one forest), "ensemble_contracted_launches" (fused launches over the contracted forests),
   "ensemble_nodes_pruned" (splits the current plan's contraction removed), "ensemble_node_steps_per_txn" (tree levels
   walked per transaction by the last fused pair launch), "ensemble_dense_chunks" (chunks of that launch over both
   forests when it walked the dense chunk stream, else 0), "forest_sparse_launches" (launches of the sparse-layout forest kernel),
   "forest_shap_launches" (launches of the TreeSHAP kernel, fd_forest_shap_*),
   "gbdt_hist_launches" (launches of the GBDT fit's histogram kernel: one per tree level), "gbdt_trees" (trees grown
   on the device by fd_gbdt_fit_* / fd_gbdt_grow_tree_*), "gbdt_nodes_split" (split nodes of those trees),
   "gbdt_eval_launches" (launches of the GBDT fit's eval kernel that walked a tree: one per round that ran with an
   eval set), "gbdt_rounds_run" (rounds the device fits ran; of a fit that
   stopped early, the launches that returned at the stop flag count in neither this, "gbdt_trees", "gbdt_hist_launches"
   nor "gbdt_eval_launches"),
   "iforest_fit_trees" (IsolationForest trees grown on the device by fd_iforest_fit_device / _host /
   _grow_tree_host), "iforest_fit_nodes_split" (split nodes of those trees),
   "mlp_fit_steps" (optimiser steps of the MLP fits), "mlp_fit_launches" (launches of the fit's step and update
   kernels: 2 per step),
   "mlp_launches" (launches of the MLP head's kernel), "graph_steps" (fd_graph_step_* calls with n > 0),
   "text_calls" (fd_text_features_device / _host calls with n > 0), "text_nonascii_rows" (rows those calls flagged
   FD_TEXT_NONASCII; reading it waits for the engine stream),
   "device_bytes_live" (bytes of device memory the library holds now, over every engine of the process: it falls
   back to its earlier value when an engine is destroyed, and reads the same through any engine),
   "pipelined_slot_stream_batches" (of those, with the slot pass on
   its own stream), "pipelined_host_ns" (host nanoseconds inside fd_score_batch_pipelined), "sharded_steps" (fd_sharded_step calls), "rccl_ops" (RCCL operations the exchanges issued: sends, receives,
   all-gathers) and "sharded_host_ns_<phase>" (host
   nanoseconds inside fd_sharded_step by phase: "wait" the split sizes, "partition" / "counts" / "count_copy" the
   next batch's route kernels, count exchange and copy to the host, "records" the records exchange, "score" the
   owner's pipeline launches, "back" / "scatter" the results exchange and the scatter into arrival order). */
int fd_engine_get_counter(fd_engine* eng, const char* key, int64_t* value);
int fd_timing_read(fd_engine* eng, int kind, double* total_ms, int64_t* launches);
int fd_timing_reset(fd_engine* eng);

#ifdef __cplusplus
}
#endif
#endif /* FDENGINE_H */

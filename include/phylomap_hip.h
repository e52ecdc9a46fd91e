/*
 * phylomap_hip.h -- C-ABI of the MI355X-native stochastic-mapping engine.
 *
 * This is the drop-in boundary for the hot path of vnminin/phylomap: the `.Call` layer
 * (src/RcppExports.cpp:9-259, R/RcppExports.R:4-50) binds `phylomap_maketreelist*`; an Rcpp shim
 *  unpacks the SEXPs into the plain structs below and calls the `phm_maketreelist*`
 * entry points, which replace the C++ drivers of src/phylomap.cpp one for one.
 *
 * Conventions
 *  - plain C: pointers + sizes, no C++/R/torch types;
 *  - all inputs are HOST buffers owned by the caller, read-only (the reference aliases and, in the
 *    Q-updating variants, mutates R's memory -- src/phylomap.cpp:917,1212-1217; this library copies);
 *  - matrices follow R's layout (COLUMN-major): Q, B, lefts, rights, d, edge, and the result;
 *  - every call returns a phm_status; phm_last_error() gives a thread-local message
 *    (the reference throws through BEGIN_RCPP/END_RCPP, src/RcppExports.cpp:35,53);
 *  - randomness: Philox4x32-7 keyed by phm_options.seed, counter (block, entity, iteration,
 *    replica), draw d = word d & 3 of block d >> 2 mapped to (x + 0.5) 2^-32; the Rcpp shim draws the seed from R's stream inside its RNGScope
 *    (src/RcppExports.cpp:38) so set.seed() still controls results;
 *  - there is NO CPU fallback: without a usable HIP device every compute call returns
 *    PHM_ERR_NO_DEVICE.
 */
#ifndef PHYLOMAP_HIP_H
#define PHYLOMAP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHM_VERSION 300     /* 300: phm_options.n_devices / devices[] (replica sharding over the GPUs of a node inside the one-shot
                                   calls); the measurement / test aids moved out of phm_options into the struct
                                   phm_debug_options, set by phm_set_debug_options.  200: named option fields instead of reserved[6]; phm_info.recoveries */
#define PHM_MAX_DEVICES 8   /* GPUs of one node (MI355X: 8 per node over xGMI) */

typedef enum phm_status {
  PHM_OK = 0,
  PHM_ERR_BAD_INPUT = 1,      /* malformed tree / model / sizes (reference: no validation at all) */
  PHM_ERR_UNSUPPORTED = 2,    /* e.g. a state count this build has no kernel for */
  PHM_ERR_NO_DEVICE = 3,      /* no HIP device, or a HIP call failed */
  PHM_ERR_OOM = 4,            /* device memory */
  PHM_ERR_ZERO_PROB = 5,      /* all-zero / non-finite probability vector (RcppArmadillo::sample throws) */
  PHM_ERR_CAPACITY = 6,       /* a sweep outgrew its dwell capacity and could not be recovered (recovery switched off, larger slots
                                 do not fit in HBM, or the 128-segment scratch of the state-per-lane tile kernel, PHM_MAP_REPLICAS with
                                 n > 4); std::list in the reference is unbounded.  After a FAILED recovery the handle has no device
                                 state left: every later call on it returns this status until it is destroyed */
  PHM_ERR_UNIF_CAP = 7,       /* newunifSample needed > 300 jumps (src/phylomap.cpp:120-125) */
  PHM_ERR_STATE = 8           /* API misuse (engine not created, iteration range, ...) */
} phm_status;

/* which exported driver of src/phylomap.cpp the engine stands in for */
typedef enum phm_variant {
  PHM_MCMC = 0,               /* maketreelistMCMC          src/phylomap.cpp:891-935  */
  PHM_MCMC_BIGTREE = 1,       /* maketreelistMCMC_bigtree  src/phylomap.cpp:942-986  (row-normalised PL, :525) */
  PHM_MCMC_SPARSE = 2,        /* SPARSEmaketreelistMCMC    src/phylomap.cpp:822-870  (B entries <= 1e-7 dropped, :811) */
  PHM_MCMC_KS = 3             /* the TREE SWEEP of maketreelistMCMCks (treesampleks :1422-1432) with Q held fixed: hidden-rates
                                 Q of even size n = 2k+2, parity tip masks (:1838-1845), tips re-sampled (:1384-1397), all
                                 consecutive state pairs counted into n x n counters (shortenerbf :1010-1014).  Result layout
                                 man/sumstatMCMCks.Rd:19: N x (n + n*n + 2 + 3k + 1): dwell, counts (row-major from,to),
                                 l01, l10, rkappas, lkappas, gammas (recordQks :1789-1798), root state (0-based).
                                 The per-iteration Gibbs/MH updates of Q (:1862-1866) run in phm_maketreelistMCMCks. */
  ,
  PHM_MCMC_BF = 4             /* tree sweep of maketreelistMCMCbf (treesamplebf :1169-1179): tips observed, n x n counts incl. self
                                 pairs (shortenerbf :1010-1014), row-normalised pruning (:1085); n-generic in the reference.  Result:
                                 N x (n + n*n + 3): dwell, counts (row-major from,to), Q[0,1], Q[1,0], root state -- at n = 2 the
                                 reference's time0,time1,n00,n01,n10,n11,l01,l10,root_state (R/sumstatMCMCbf.R:33; its column 8 is
                                 hard-wired at :1129, which is n + n*n + 2 for two states).  The rate updates (two states only)
                                 run in phm_maketreelistMCMCbf */
  ,
  PHM_MCMC_MT = 5             /* tree sweep of maketreelistMCMCmt (treesamplemtNS :2157-2165): the bf sweep with the UN-normalised
                                 pruning makePLrcppmt :1938-1950; two states */
  ,
  PHM_MCMC_KSMT = 6           /* tree sweep of maketreelistMCMCksmt (:2722-2844): the ks sweep with the un-normalised pruning */
} phm_variant;

/* The phylomap tree object `x` (fields read at src/phylomap.cpp:896-910 and :3034). */
typedef struct phm_tree {
  int32_t n_tips;              /* length(x$states) */
  int32_t n_node;              /* x$Nnode (= n_tips-1: strictly bifurcating, :508-510) */
  int32_t n_edge;              /* nrow(x$edge) */
  const int32_t* edge;         /* n_edge x 2 column-major, 1-based (parent, child); tips are 1..n_tips (:904) */
  const double*  edge_length;  /* x$edge.length (:3034); EXP only, may be NULL for MCMC */
  const int32_t* states;       /* x$states, 1-based (:910); n_tips values, or n_replicas*n_tips when
                                  phm_options.tips_per_replica != 0 (replica-major) */
  const int32_t* map_off;      /* n_edge+1 offsets into maps/mapnames */
  const double*  maps;         /* x$maps flattened: dwell times per segment (:896) */
  const int32_t* mapnames;     /* x$mapnames flattened: 1-based states (:897, :29) */
} phm_tree;

typedef struct phm_model {
  int32_t n_states;            /* n = nrow(Q) */
  const double* Q;             /* n x n rate matrix, column-major */
  const double* pid;           /* n root prior */
  const double* B;             /* n x n, I + Q/Omega (R/sumstatMCMC.R:25), column-major; NULL -> computed */
  double Omega;                /* dominating rate; must exceed every |q_ii| (man/sumstatMCMC.Rd:14) */
  int32_t variant;             /* phm_variant */
} phm_model;

/* how a sweep is laid over the lanes (phm_options.mapping).  n <= 4: REPLICAS = one lane per replica, one wave per 64-replica
 * tile walks the tree (largest replica counts); BRANCHES = the sweep of one chain spread over the device for latency (one chain or a handful, large trees);
 * TILES = one wave per (64-replica tile, branch) (10^2 .. 10^5 replicas).  5..64 states: REPLICAS = one wave per 64-replica
 * tile, replicas in turn, lanes = states (phm_wide.hip; lists of trees); BRANCHES = one wave per (replica, branch), lanes =
 * states (a handful of chains); TILES = one lane per replica, one wave per (tile, item), pruning on the matrix cores or over
 * the non-zeros of a sparse B (the default beyond 50 000 / n_edge chains, clamped to 1..32: the measured crossover).
 * phm_maketreelistEXP: AUTO / TILES = one wave per (tile of 64 samples, branch); REPLICAS = one wave per tile of 64 samples
 * walks the tree (dwell sums then add in the reference's order). */
typedef enum phm_mapping { PHM_MAP_AUTO = 0, PHM_MAP_REPLICAS = 1, PHM_MAP_BRANCHES = 2, PHM_MAP_TILES = 3 } phm_mapping;

typedef struct phm_options {
  uint64_t seed;               /* Philox key */
  int32_t n_replicas;          /* S: independent chains / sites run side by side (>=1; 0 -> 1) */
  int32_t replica_offset;      /* global id of this device's first replica (multi-GPU sharding) */
  int32_t reduce;              /* 0: statistics per replica; 1: summed over replicas per iteration */
  int32_t tips_per_replica;    /* 0: all replicas share x$states; 1: one tip vector per replica (sites) */
  int32_t device;              /* HIP device ordinal; -1 = current device */
  int32_t iters_per_launch;    /* MCMC iterations fused into one kernel launch; 0 -> default */
  double  cap_tail;            /* dwell capacity: the 1+Poisson(Omega*t_b) quantile at this tail, per branch.  0 -> automatic: 1e-3 for
                                  the sequential streams of PHM_MAP_REPLICAS (an overflow there is rare per TILE and recovered); for the
                                  fixed slots of PHM_MAP_BRANCHES / PHM_MAP_TILES min(1e-9, 0.05 / (S * E * max_iters)), floored at
                                  1e-16 -- at most 0.05 expected recoveries over the draws the engine is created for, so the HBM
                                  held per replica grows (slowly: a quantile) with max_iters */
  int32_t mapping;             /* phm_mapping: how a sweep is laid over the lanes (one tree); PHM_MAP_AUTO = by replica count.
                                  Same draws and counts in every mapping; dwell sums differ in the last bits between
                                  PHM_MAP_REPLICAS and the other two (summation order).  Path lengths: 65 535 segments per branch
                                  in PHM_MAP_TILES, slot sizes in PHM_MAP_BRANCHES; PHM_MAP_REPLICAS with 5..64 states (never the
                                  automatic choice for one tree) holds at most 128 segments per branch and replica and answers
                                  PHM_ERR_UNSUPPORTED / PHM_ERR_CAPACITY beyond. */
  int32_t storage;             /* dwell-stream storage of PHM_MAP_REPLICAS: 0 = automatic, 1 = one ring per tile (half the HBM),
                                  2 = two buffers (5 % faster sweep for n <= 4) */
  int32_t rescale_pruning;     /* phm_maketreelistEXP: 1 = divide every internal partial-likelihood row by its sum in the pruning
                                  pass.  The reference's makePLexp (src/phylomap.cpp:2899-2906) does not rescale, so sumstatEXP
                                  underflows (PHM_ERR_ZERO_PROB) beyond a few hundred tips; node draws do not depend on a row's
                                  scale, so this is the same sampler in exact arithmetic.
                                  phm_maketreelistMCMC / phm_SPARSEmaketreelistMCMC: 1 = the same for their pruning pass (what
                                  makePLrcpp_bigtree :525 does; the plain and the SPARSE driver underflow on trees of thousands
                                  of tips, man/sumstatMCMC_bigtree.Rd:17) */
  int32_t no_recovery;         /* 1 = a sweep that outgrows its slots fails with PHM_ERR_CAPACITY.  Default (0): the engine is
                                  rebuilt with doubled slots and the iterations run so far are replayed -- bit-identical, every
                                  random number being addressed by (replica, iteration, entity) -- so a run cannot abort where
                                  the reference's std::list (src/phylomap.cpp:18-21) would grow */
  int32_t sparse_chains;       /* 5..64 states with PHM_MAP_TILES: pruning chains and forward draws over the NON-ZEROS of B only
                                  (what SPARSEmakePLrcpp :490-501 / SPARSEresamplebranchstates :218-261 get from sp_mat).  0 =
                                  automatic: used when n <= 32 and B has a half-bandwidth of 1 (tridiagonal) or 2 (make2sQ hidden
                                  rates), or is sparse enough for the pattern-specialised kernels; 1 = required
                                  (PHM_ERR_UNSUPPORTED otherwise); 2 = never (chains on the matrix cores).
                                  Same bits either way: a skipped term is an exact zero */
  int32_t n_devices;           /* one-shot calls (phm_maketreelist*): 0 / 1 = one GPU (`device`); 2..PHM_MAX_DEVICES = the
                                  n_replicas chains / sites (phm_maketreelistEXP: the N samples) are sharded by GLOBAL replica id
                                  over devices[0 .. n_devices-1], one host thread and one engine per device, no traffic between
                                  the devices while sampling; with reduce = 1 the per-tile sums are folded in device order (the
                                  only exchange: N x cols doubles per device).  Every random number is addressed by the global
                                  replica id, so counts are those of ONE device exactly and dwell sums agree to rounding
                                  (<= 1e-12; bit-identical on the mappings whose per-tile sums do not depend on the tile count).
                                  The resident engine (phm_engine_*) is per device: shard with replica_offset there.
                                  The caller of the reference -- R/sumstatMCMC_bigtree.R:21-29 -> .Call -> one function
                                  (src/phylomap.cpp:942-986) -- reaches all GPUs of the node through this field */
  int32_t devices[PHM_MAX_DEVICES]; /* HIP ordinals; an ordinal may repeat (several engines on one GPU: rehearsal on a one-GPU box) */
  int32_t reserved[3];         /* must be 0 */
} phm_options;

/* Measurement and test aids, kept out of phm_options: set per THREAD by phm_set_debug_options and read by the engines and
 * one-shot calls that thread creates afterwards (NULL resets to all-zero). */
typedef struct phm_debug_options {
  int32_t pruning_form;        /* 5..64 states with PHM_MAP_TILES: form of the pruning kernel, 0 = by tile count, 1 = one wave per
                                  (node, tile) with the chain matrix in registers, 2 = one workgroup / wave per 16-replica block,
                                  3 = one wave per (node, tile) with the chain matrix in LDS and two waves per SIMD (33..64 states;
                                  what 0 chooses there from 192 / 256 tiles on) (same bits).
                                  2..4 states with PHM_MAP_BRANCHES: the subtree clusters of the pruning sweep, 0 = by path length
                                  (some branch expected to hold >= 96 segments: dependency-driven), 1 = a barrier per tree level,
                                  2 = dependency-driven (same bits) */
  int32_t phase_timing;        /* 1 = record HIP events between the phases of a sweep (phm_engine_phase_ms) */
  int32_t fail_recovery;       /* 1 = every capacity recovery "does not fit" (exercises the dead-handle path) */
  int32_t branch_group;        /* (tile, branch) mapping, 2..64 states: > 0 = branches per wave of the branch kernel (clamped to
                                  1..64); 0 = automatic (tiles x branches / 65 536, at most 16 for 2..4 states and 8 beyond).  Counts
                                  and integer columns do not depend on it; dwell sums are rounded per group */
  int32_t level_groups;        /* (tile, branch) mapping, n <= 4 (5..32 states: 2 / 3 = the node draws and the band pruning kernel over
                                  subtree clusters; automatic on a deep tree): tree passes over clusters of tree levels (one launch per tier of eight
                                  levels) instead of one launch per level: 0 = automatic (tiles x internal nodes <= 65 536; a deep, ladder-like
                                  tree at any tile count, with clusters cut by subtree size), 1 = never, 2 = always, 3 = always with
                                  clusters cut by subtree size.  Same bits */
  int32_t q_timing;            /* 1 = the rate-updating drivers print the mean host time of the phases of an iteration to stderr */
  double  pade_pivot_min;      /* > 0: smallest pivot phm_expm_pade_mfma's unpivoted block elimination accepts (default 1e-3;
                                  1e300 sends every matrix to the pivoted kernel) */
  int32_t expect_chunk;        /* > 0: phm_expected_stats and phm_expected_through_time run at most this many sites (rounded up to
                                  64) per pass and this many branches, points or sub-branches per launch (default 0: sites by free
                                  HBM, the rest by a 256 MB scratch); the results do not depend on it */
  int32_t sweep_parts;         /* (tile, branch) mapping, n <= 4, one launch per tree level: contiguous groups of tiles whose sweeps
                                  phm_engine_run issues on streams of their own (part 0 on the caller's), so that the narrow tree levels
                                  and reductions of one part run beside the branch kernel of another: 0 = automatic, 1 .. 4 = forced
                                  (never more parts than tiles).  Same bits.  With more than one part the phase times of
                                  phm_engine_phase_ms are summed over parts that share the chip and exceed last_run_ms */
  int32_t reserved[2];
} phm_debug_options;

typedef struct phm_info {
  int32_t n_states, n_edge, n_replicas, n_replicas_padded, n_cols, max_iters;
  int64_t device_bytes;        /* HBM held by the engine */
  int64_t rows_per_replica;    /* capacity (64-lane rows) of one tile's dwell storage */
  int64_t seg_read;            /* sum over branches x valid replicas x iterations run so far of (m_b + m'_b): segments
                                  read plus segments written; feeds the algorithmic-bytes figure of bench.py */
  int64_t seg_written;         /* reserved (0) */
  double  last_run_ms;         /* HIP-event time of the last phm_engine_run (all its launches) */
  int32_t last_run_launches;
  int32_t iters_done;
  int32_t recoveries;          /* capacity recoveries (rebuild + replay) this handle has gone through; a timed region asserts 0 */
  int32_t mapping;             /* the phm_mapping in force (the automatic choice resolved) */
  int32_t sparse_chains;       /* bit 0: pruning chains run over the non-zeros of the chain matrix; bit 1: forward draws over the band of B;
                                  bit 2: the pruning kernel was generated for the matrix's pattern (unstructured sparsity, hipRTC) */
  int32_t reserved;
} phm_info;

typedef struct phm_engine phm_engine;

/* ---- library ---- */
int32_t     phm_version(void);
/* sizeof of the plain structs of this header as the library was built (which: 0 phm_options, 1 phm_info, 2 phm_tree,
 * 3 phm_model, 4 phm_debug_options; anything else: -1) -- lets a foreign-function binding (ctypes, cgo, .C) check its mirror of the layout */
int32_t     phm_struct_size(int32_t which);
int32_t     phm_device_count(void);
const char* phm_last_error(void);
const char* phm_status_string(int32_t status);
/* measurement / test aids of this thread -- see the phm_debug_options struct; NULL = defaults */
int32_t     phm_set_debug_options(const phm_debug_options* dbg);
/* measurement aid: HIP-event milliseconds of the sampling kernel of this thread's last phm_maketreelistEXP call (or of the
 * simulation kernel of its last forward simulation) */
double      phm_last_kernel_ms(void);

/* ---- reference-shaped one-shot entry points (what the Rcpp shim binds) ----
 * Each mirrors the argument list of the exported C++ driver it replaces; `out` is the caller-allocated
 * N x (n + n(n-1)) column-major result (allocMatrix(REALSXP, N, cols) in the shim).  With
 * opt->n_replicas = S > 1 and reduce = 0, `out` holds S such matrices back to back.
 * nen / nodelist / root (R/sumstatMCMC.R:1-18) are checked for consistency with `x->edge`
 * and otherwise unused: the engine derives its own O(E) sweep schedules. */
int32_t phm_maketreelistMCMC(         /* src/phylomap.cpp:891, src/RcppExports.cpp:34 */
    const phm_tree* x, int32_t n_states, const double* Q, const double* pid, const double* B, double Omega,
    const int32_t* nen, const int32_t* nodelist, int32_t root, int32_t N,
    const phm_options* opt, double* out);
int32_t phm_maketreelistMCMC_bigtree( /* src/phylomap.cpp:942, src/RcppExports.cpp:57 */
    const phm_tree* x, int32_t n_states, const double* Q, const double* pid, const double* B, double Omega,
    const int32_t* nen, const int32_t* nodelist, int32_t root, int32_t N,
    const phm_options* opt, double* out);
int32_t phm_SPARSEmaketreelistMCMC(   /* src/phylomap.cpp:822, src/RcppExports.cpp:11 */
    const phm_tree* x, int32_t n_states, const double* Q, const double* pid, const double* B, double Omega,
    const int32_t* nen, const int32_t* nodelist, int32_t root, int32_t N,
    const phm_options* opt, double* out);
/* Tree sweep of sumstatMCMCks with Q held fixed (see PHM_MCMC_KS); out: N x (n + n*n + 2 + 3k + 1) column-major. */
int32_t phm_maketreelistMCMCks_sweep( /* src/phylomap.cpp:1802 minus the Q updates of :1862-1866 */
    const phm_tree* x, int32_t n_states, const double* Q, const double* pid, const double* B, double Omega,
    const int32_t* nen, const int32_t* nodelist, int32_t root, int32_t N,
    const phm_options* opt, double* out);
/* Tree sweep of sumstatMCMCbf with Q held fixed (see PHM_MCMC_BF), ANY n: tips observed, all consecutive pairs counted
 * (the "n + n^2" layout of shortenerbf); out: N x (n + n*n + 3) column-major: dwell, counts (row-major from,to), Q[0,1], Q[1,0],
 * root state (0-based). */
int32_t phm_maketreelistMCMCbf_sweep( /* treesamplebf src/phylomap.cpp:1169-1179 inside the N-loop of :1295-1301, minus the updates */
    const phm_tree* x, int32_t n_states, const double* Q, const double* pid, const double* B, double Omega,
    const int32_t* nen, const int32_t* nodelist, int32_t root, int32_t N,
    const phm_options* opt, double* out);
/* The Q-updating drivers: tree sweep on the device + Gibbs/MH update of the rate matrix on the host, every iteration.
 * bf: two states, prior = c(a01,b01,a10,b10), out N x 9 (R/sumstatMCMCbf.R:33).  ks: n = 2k+2 >= 4,
 * prior = c(a_l,b_l,a_k,b_k,a_g,b_g), out N x (n+n*n+2+3k+1) (man/sumstatMCMCks.Rd:19).  Inputs are never written
 * (the reference edits the caller's Q and B in place, src/phylomap.cpp:1212-1217).  Gamma variates: Marsaglia-Tsang on the
 * Philox stream (R's Rf_rgamma is third-party code).  With S > 1 replicas (sites sharing Q) the updates see, and `out`
 * holds, the statistics summed over sites. */
int32_t phm_maketreelistMCMCbf(       /* src/phylomap.cpp:1258, src/RcppExports.cpp:106 */
    const phm_tree* x, int32_t n_states, const double* Q, const double* pid, const double* B, double Omega,
    const int32_t* nen, const int32_t* nodelist, int32_t root, int32_t N, const double* prior, int32_t n_prior,
    const phm_options* opt, double* out);
int32_t phm_maketreelistMCMCks(       /* src/phylomap.cpp:1802, src/RcppExports.cpp:132 */
    const phm_tree* x, int32_t n_states, const double* Q, const double* pid, const double* B, double Omega,
    const int32_t* nen, const int32_t* nodelist, int32_t root, int32_t N, const double* prior, int32_t n_prior,
    const phm_options* opt, double* out);
/* The DIC drivers: the bf / ks drivers plus log p(y|Q) by matrix exponentiation every iteration (expmat(Q t_b) for every
 * branch -- Pade scaling-and-squaring on the device -- then pruning with scale factors in nen order), appended as the last
 * column: out is N x 10 (2sDICt) or N x (n+n*n+2+3k+2) (ksDICt).  One chain (n_replicas = 1); needs x->edge_length. */
int32_t phm_maketreelistMCMC2sDICt(   /* src/phylomap.cpp:3183, src/RcppExports.cpp:211 */
    const phm_tree* x, int32_t n_states, const double* Q, const double* pid, const double* B, double Omega,
    const int32_t* nen, const int32_t* nodelist, int32_t root, int32_t N, const double* prior, int32_t n_prior,
    const phm_options* opt, double* out);
int32_t phm_maketreelistMCMCksDICt(   /* src/phylomap.cpp:3300, src/RcppExports.cpp:237 */
    const phm_tree* x, int32_t n_states, const double* Q, const double* pid, const double* B, double Omega,
    const int32_t* nen, const int32_t* nodelist, int32_t root, int32_t N, const double* prior, int32_t n_prior,
    const phm_options* opt, double* out);
/* The multi-tree drivers: `trees` is the R list x of `n_trees` phylomap trees with equal tip and edge counts
 * (R/sumstatMCMCmt.R:33-35).  Every iteration sweeps every tree with the current Q -- one launch, tree j on replica tile j --
 * draws one tree uniformly, writes that tree's row plus its 0-based index (the last column; R/sumstatMCMCmt.R:41
 * "tree_number") and updates Q from it with the mt twins of the updates (updatel01mtNS :2192, updateksl01mt :2371, ...).
 * nen_m: n_trees x 2*Nnode, nodelist_m: n_trees x (Nnode-1), both COLUMN-major as R passes its matrices; either may be
 * NULL (orders are derived from edge; when given they are checked against it).  out: N x (n+n*n+2+3k+1) column-major.
 * prior: 4 numbers (mt), 8 (ksmt: l01, l10, kappas, gammas shape/rate pairs as the mt updates index them). */
int32_t phm_maketreelistMCMCmt(       /* src/phylomap.cpp:2267, src/RcppExports.cpp:158 */
    const phm_tree* trees, int32_t n_trees, int32_t n_states, const double* Q, const double* pid, const double* B,
    double Omega, const int32_t* nen_m, const int32_t* nodelist_m, const int32_t* roots, int32_t N, const double* prior,
    int32_t n_prior, const phm_options* opt, double* out);
int32_t phm_maketreelistMCMCksmt(     /* src/phylomap.cpp:2722, src/RcppExports.cpp:184 */
    const phm_tree* trees, int32_t n_trees, int32_t n_states, const double* Q, const double* pid, const double* B,
    double Omega, const int32_t* nen_m, const int32_t* nodelist_m, const int32_t* roots, int32_t N, const double* prior,
    int32_t n_prior, const phm_options* opt, double* out);
int32_t phm_maketreelistEXP(          /* src/phylomap.cpp:3001, src/RcppExports.cpp:80 */
    const phm_tree* x, int32_t n_states, const double* Q, const double* pid,
    const int32_t* nen, const int32_t* nodelist, int32_t root, int32_t N,
    const double* lefts, const double* rights, const double* d,
    const phm_options* opt, double* out);

/* ---- forward simulation: data for the samplers ----
 * Forward simulation of the chain along the tree (R/sourceme.R:346-414, sample2statehistory / samplethebranch), n_replicas
 * independent histories.  Reads x->edge, x->edge_length, n_tips, n_node only (states / maps may be NULL).
 * observe: NULL = identity, else n values in 1..n: the tip state reported for each true state (simulate_4_state_tree's
 * parity map is {1,2,1,2}).  tips: n_replicas x n_tips, REPLICA-major, 1-based (the layout of x->states with
 * tips_per_replica = 1).  nodes: NULL, or n_replicas x (n_tips + n_node), replica-major, 1-based true states by ape node id.
 * stats: n_replicas x (n + n*n + 1) column-major: dwell per state, jump counts n x n row-major (from,to) with zero diagonal,
 * root state (0-based).
 * Options: seed, n_replicas, replica_offset, device, n_devices / devices[] (sharded by global replica id); reduce must be 0;
 * mapping is ignored.  2 <= n <= 64; Q with finite off-diagonal entries >= 0 and rows summing to 0 (1e-12 max|q|); pid >= 0
 * with a positive sum (else PHM_ERR_ZERO_PROB).  A branch that needs more than 9 999 jumps (where samplethebranch stops,
 * R/sourceme.R:356) fails with PHM_ERR_CAPACITY naming its edge row; an absorbing state (q_ss = 0) keeps the rest of the
 * branch.  Random numbers: DESIGN.md section 12 (Philox iteration word 0xFFFFFFFF, which no MCMC sweep reaches).
 * phm_last_kernel_ms gives the simulation kernel's time. */
int32_t phm_simulate_histories(const phm_tree* x, int32_t n_states, const double* Q, const double* pid,
                               const int32_t* observe, const phm_options* opt,
                               int32_t* tips, int32_t* nodes, double* stats);

/* ---- stochastic maps of sampled and simulated histories ----
 * phm_simulate_histories / phm_maketreelistEXP that also return each history: R histories (n_replicas simulations, N EXP samples)
 * over the E = n_edge edge rows.  Row k = r * E + b (0-based, edge-row order) is history r's map on edge row b: segments
 * [map_off[k], map_off[k+1]) of map_dwell (time) and map_state (1-based, the mapnames convention), from the parent end to the
 * child end; the first segment has the parent's state, the last the child's (TRUE states for the simulator, whatever `observe`
 * reports), consecutive segments differ, and each dwell is the double the sampler adds to its statistics.  One history's rows
 * are a phm_tree map_off / maps / mapnames triple once its offsets are rebased to 0 and narrowed to int32.
 * Two phases, no state kept between calls:
 *   sizing  (map_dwell == map_state == NULL): the usual call, and map_off (R*E + 1 int64, map_off[0] = 0) is written;
 *   filling (both non-NULL): map_off is READ (from a sizing call with the same inputs and seed: draws are addressed by (seed,
 *           entity, replica), so the same inputs give the same histories); map_cap >= map_off[R*E] is required; the segments are
 *           written and every other output is bit-identical to the sizing call.  A row whose segment count differs from map_off
 *           gives PHM_ERR_BAD_INPUT naming the first such row; nothing outside a row's [map_off[k], map_off[k+1]) is written.
 * Every other argument means what it means for the plain entry point and gives the same bits; n_devices / devices[] shard the
 * histories and every output is the one-device output bit for bit.  Checks, all before any device call: map_off non-NULL,
 * R*E + 1 offsets addressable, and when filling: map_off[0] = 0, never decreasing, map_off[R*E] <= map_cap.  Segments that do not
 * fit in free HBM: PHM_ERR_OOM with the size.  Segment counts: at most 10 000 per row (simulator), 301 (EXP).
 * phm_maketreelistEXP_maps runs the (tile, branch) kernels: mapping PHM_MAP_AUTO or PHM_MAP_TILES, anything else is
 * PHM_ERR_UNSUPPORTED; rescale_pruning is honoured.  phm_last_kernel_ms: the sampling kernel plus, when sizing, the offsets scan. */
int32_t phm_simulate_histories_maps(const phm_tree* x, int32_t n_states, const double* Q, const double* pid,
                                    const int32_t* observe, const phm_options* opt,
                                    int32_t* tips, int32_t* nodes, double* stats,
                                    int64_t* map_off, int64_t map_cap, double* map_dwell, int32_t* map_state);
int32_t phm_maketreelistEXP_maps(const phm_tree* x, int32_t n, const double* Q, const double* pid, const int32_t* nen,
                                 const int32_t* nodelist, int32_t root, int32_t N, const double* lefts, const double* rights,
                                 const double* d, const phm_options* opt, double* out,
                                 int64_t* map_off, int64_t map_cap, double* map_dwell, int32_t* map_state);

/* ---- stochastic maps of the MCMC samplers ----
 * The fixed-Q one-shot drivers (variant PHM_MCMC, PHM_MCMC_BIGTREE, PHM_MCMC_SPARSE, PHM_MCMC_KS or PHM_MCMC_BF; anything else is
 * PHM_ERR_UNSUPPORTED) that also return the chains' sampled histories at the iterations map_iters: J >= 1 strictly increasing
 * 0-based values below N, or NULL with n_map_iters = 0 for every iteration (J = N); S * J must fit in int32 (S = n_replicas).
 * History h = s * J + j is chain s at iteration map_iters[j]; row k = h * E + b its map on edge row b, in the format and with the
 * two-phase contract of the section 14 entry points above (map_off holds S*J*E + 1 offsets).  The map of a row is the path that
 * iteration's branch step makes of the branch after its interior states are resampled and equal neighbours merged, before the
 * virtual jumps are re-inserted: the first segment has the parent's state (the child's throughout on a branch of one old segment:
 * updatenodestates' "child wins"), the last the child's (a tip's observed state; with PHM_MCMC_KS the hidden state sampled that
 * iteration), consecutive segments differ, each dwell is the sum of the old segments it merges, added left to right.  The
 * transitions between consecutive segments of history (s, j), summed over its rows, are the off-diagonal counts of row
 * map_iters[j] of chain s in `out`.  At most 65 535 segments per row.  mapping: PHM_MAP_AUTO or PHM_MAP_TILES (the (tile, branch)
 * kernels run either way), anything else is PHM_ERR_UNSUPPORTED; every other argument and option means what it means for the
 * plain driver of the variant (sites, reduce, cap_tail, no_recovery, devices).  `out` is bit-identical to the plain driver's with
 * mapping = PHM_MAP_TILES; its counts equal the plain driver's under any mapping.  Every argument check runs before any device call.
 * phm_last_kernel_ms: the device time of the sweeps, the replays included. */
int32_t phm_maketreelistMCMC_maps(int32_t variant, const phm_tree* x, int32_t n_states, const double* Q, const double* pid,
                                  const double* B, double Omega, const int32_t* nen, const int32_t* nodelist, int32_t root, int32_t N,
                                  const int32_t* map_iters, int32_t n_map_iters, const phm_options* opt, double* out,
                                  int64_t* map_off, int64_t map_cap, double* map_dwell, int32_t* map_state);

/* ---- exact conditional expectations given the tips ----
 * For a fixed Q, per site (one tip vector): E[dwell_i | tips], E[N_ij | tips] summed over the tree and per branch, log p(tips | Q)
 * and P(state of node k | tips), by an up (pruning) pass, a down (outside) pass and one uniformization integral per branch
 * (Minin & Suchard 2008).  No sampling: the numbers every sampler's posterior mean converges to.
 * Reads x->edge, x->edge_length, n_tips, n_node and x->states: n_tips values shared by every site (tips_per_replica = 0) or
 * n_replicas x n_tips replica-major (tips_per_replica = 1).  A tip state is 0 (missing: every state allowed) or a value y in 1..n;
 * the tip vector is 1 for the states a with observe[a] == y (observe NULL = identity).  pid: root prior (normalised here).
 * Outputs, column-major with the site index fastest (R's array(dim = c(S, ...))), S = n_replicas sites:
 *   stats: S x (n + n(n-1)): n dwell columns, then the off-diagonal counts in man/sumstatMCMC.Rd:18 order (1->2, 1->3, .., n->n-1);
 *   loglik: S values; branch_stats: NULL or S x n_edge x (n + n(n-1)) by edge row; node_post: NULL or S x (n_tips + n_node) x n
 *   by ape node id.
 * Options: n_replicas, tips_per_replica, device, n_devices / devices[] (sharded by global site id; every row is the one-device
 * row bit for bit); reduce must be 0; seed and replica_offset are ignored.  2 <= n <= 64; Q finite, off-diagonal >= 0, rows
 * summing to 0 (1e-12 max|q|), some q_ii < 0; pid >= 0 with a positive sum; a strictly bifurcating tree with finite
 * non-negative edge lengths and max(-q_ii) * t_b <= 1e6.  Every check runs before any device call.  A site whose tips are
 * impossible under Q returns PHM_ERR_ZERO_PROB naming the site.  phm_last_kernel_ms: device time of the passes and the
 * branch stage. */
int32_t phm_expected_stats(const phm_tree* x, int32_t n_states, const double* Q, const double* pid,
                           const int32_t* observe, const phm_options* opt,
                           double* stats, double* loglik, double* branch_stats, double* node_post);

/* ---- exact state probabilities and expected statistics through time ----
 * For a fixed Q, per site: WHEN things happen.  Depth runs from the root: d(root) = 0, d(child) = d(parent) + t_b (double, down-pass
 * order).  Tree, tips, Q, pid, observe, options and limits are phm_expected_stats' and checked the same way.  Outputs, column-major
 * with the site index fastest (S = n_replicas sites); at least one must be non-NULL:
 *   occupancy: NULL or S x n_bounds x n, the expected number of lineages in state i at depth bounds[k]: the state posterior at every
 *     branch with d_parent < bounds[k] <= d_child (a node at the bound counts once, through its parent branch; zero-length branches
 *     never count), plus the root's posterior at a bound of 0.  Summed over i it is the number of lineages at that depth.
 *   bin_stats: NULL or S x (n_bounds - 1) x (n + n(n-1)), E[dwell_i] and E[N_ij] within depths [bounds[k], bounds[k+1]) in
 *     phm_expected_stats' column order; parts of branches outside [bounds[0], bounds[n_bounds-1]) are not reported.
 *   point_post: NULL or S x n_points x n, P(state at the point | tips) for the point at distance point_pos[p] from the parent end of
 *     0-based edge row point_edge[p] (0 <= point_pos[p] <= t_b: the parent's and the child's node posteriors at the ends).
 *   loglik: NULL or S values, phm_expected_stats' loglik bit for bit.
 * bounds: n_bounds finite values >= 0, strictly increasing; n_bounds >= 1 with occupancy, >= 2 with bin_stats (0 and NULL are
 * allowed otherwise).  point_edge / point_pos: n_points values, read and checked whenever n_points > 0; n_points >= 1 with
 * point_post.  A bad bound or point is PHM_ERR_BAD_INPUT naming its 0-based index.  Every check runs before any device call.
 * n_devices / devices[] shard the sites (every row is the one-device row bit for bit); phm_debug_options.expect_chunk caps the
 * chunks; phase_timing = 1 prints the device time of the passes, the along-branch vectors, the branch stage and the reductions to
 * stderr.  phm_last_kernel_ms: device time of all of them, P(t_b) and P(s) included. */
int32_t phm_expected_through_time(const phm_tree* x, int32_t n_states, const double* Q, const double* pid,
                                  const int32_t* observe, const phm_options* opt,
                                  int32_t n_bounds, const double* bounds,
                                  double* occupancy,   /* S x n_bounds x n, or NULL */
                                  double* bin_stats,   /* S x (n_bounds-1) x (n + n(n-1)), or NULL */
                                  int64_t n_points, const int32_t* point_edge, const double* point_pos,
                                  double* point_post,  /* S x n_points x n, or NULL */
                                  double* loglik);     /* S, or NULL */

/* ---- log-likelihood of many rate matrices in one call ----
 * log p(tips_s | Q_k, pid_k) for K models: what a maximum-likelihood fit evaluates (the points of a finite-difference gradient,
 * line-search candidates, several starts, one model per simulated dataset).  Section 13's up pass with the models across the
 * lanes (2..8 states; 9..64 states are computed one model after the other, not batched).  Tree, tips (n_replicas and
 * tips_per_replica give the S sites), observe and options as phm_expected_stats.
 *   Q: n x n x K, each matrix column-major, model slowest; checked per model like phm_expected_stats' (a bad model is
 *     PHM_ERR_BAD_INPUT naming its 0-based index), except that a model that leaves no state (P = I) is legal and there is no
 *     limit on max(-q_ii) * t_b.
 *   pid: n x n_pid root priors (normalised here), n_pid = 1 (shared) or K.
 *   site_of_model NULL ("cross"): every model on every site; out is S x K column-major (site fastest).
 *   site_of_model = K site indices in 0..S-1 ("paired"): model k on site site_of_model[k] alone; out has K values.
 * An evaluation of probability 0, or of a model for which some expm(Q_k t_b) meets a zero pivot, is -inf and does not fail the
 * call.  Every check runs before any device call.  n_devices / devices[] shard the models and phm_debug_options.expect_chunk
 * caps the chunks of models and sites; every output value is the same bit for bit whatever they are.
 * phm_last_kernel_ms: device time of the call. */
int32_t phm_loglik_models(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid, int32_t n_pid,
                          const int32_t* observe, const int32_t* site_of_model, const phm_options* opt, double* out);

/* ---- expected statistics of many rate matrices in one call ----
 * E[dwell_i | tips_s, Q_k] and E[N_ij | tips_s, Q_k], summed over the tree, with log p(tips_s | Q_k): what an exact score, an
 * observed information matrix or an EM step needs at many Q.  Section 13's passes and branch stage with the models across the
 * lanes (2..8 states; 9..64 states go one model after the other through phm_expected_stats, not batched).  Every argument up to
 * opt is phm_loglik_models', checked the same way, with two limits of phm_expected_stats kept: max(-q_ii) * t_b above 1e6 for any
 * model is PHM_ERR_UNSUPPORTED, and so is a model that leaves no state with more than 8 states.
 *   loglik: S x K values (cross, site fastest) or K values (paired): phm_loglik_models' values bit for bit.
 *   stats: n + n(n-1) columns per evaluation in phm_expected_stats' column order, column-major with the evaluation (the index
 *     into loglik) fastest.  A structurally zero q_ij gives E[N_ij] = 0; a model that leaves no state (2..8 states) gives
 *     dwell = t_b on the posterior state and zero counts.
 * An evaluation that phm_loglik_models reports as -inf gets -inf and a row of NaN and does not fail the call.  Every check runs
 * before any device call.  n_devices / devices[] shard the models and phm_debug_options.expect_chunk caps the chunks of models,
 * sites and branches; every output value is the same bit for bit whatever they are.  phm_last_kernel_ms: device time of the call. */
int32_t phm_expected_stats_models(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid,
                                  int32_t n_pid, const int32_t* observe, const int32_t* site_of_model, const phm_options* opt,
                                  double* stats, double* loglik);

/* ---- exact sampler of histories over many rate matrices and sites ----
 * D = draws independent histories per evaluation (model k, site s), each an exact draw from p(history | tips_s, Q_k, pid_k): the
 * stochastic maps under a fitted Q with its uncertainty, under per-dataset fits or under a posterior sample of Q.  Every argument
 * up to site_of_model is phm_loglik_models', checked the same way before any device call.  2..8 states (9..64:
 * PHM_ERR_UNSUPPORTED); max(-q_ii) * t_b above 32768 for any model is PHM_ERR_UNSUPPORTED naming the model.  There is no jump cap
 * below that.  An evaluation's index e is its index into loglik; history h = e * draws + d.  H = evaluations * draws.
 *   loglik: phm_loglik_models' values bit for bit.
 *   stats:  H x (n + n(n-1)), column-major with the history fastest, phm_expected_stats' column order.
 *   nodes:  NULL, or H x (n_tips + n_node) history-major: the 1-based TRUE state of every node by ape node id, tips included (a
 *           missing tip comes out sampled, and so does the hidden state behind an observe map).
 *   map_off NULL: no maps.  Otherwise the two-phase contract of phm_simulate_histories_maps with R = H: a sizing call (map_dwell
 *           and map_state NULL) writes the H * n_edge + 1 offsets, a filling call reads them; row h * n_edge + b.
 * An evaluation whose log-likelihood is -inf is not drawn: NaN rows of stats, zeros in nodes, empty map rows; it does not fail the
 * call.  Random numbers: phm_options.seed and replica_offset (added to the draw index d); every draw is addressed by the global
 * evaluation (site * n_models + model) and d, so n_devices / devices[] (which shard the models) and
 * phm_debug_options.expect_chunk (which caps the chunks of models, sites and tiles) change no output bit.
 * phm_last_kernel_ms: device time of the whole call. */
int32_t phm_sample_histories_models(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid,
                                    int32_t n_pid, const int32_t* observe, const int32_t* site_of_model, int32_t draws,
                                    const phm_options* opt, double* stats, double* loglik, int32_t* nodes,
                                    int64_t* map_off, int64_t map_cap, double* map_dwell, int32_t* map_state);

/* ---- ancestral states of many rate matrices in one call: marginal and joint ----
 * Per evaluation (model k, site s): the marginal posterior of the state of every reported node, and the JOINT reconstruction --
 * the one assignment of ALL nodes that maximises p(states of all nodes, tips_s | Q_k, pid_k) (Pupko et al. 2000: a max-product up
 * pass with back pointers, then a traceback; ties go to the smallest state, on the device's own P).  Every argument up to
 * site_of_model is phm_loglik_models', checked the same way before any device call.  2..8 states (9..64: PHM_ERR_UNSUPPORTED;
 * phm_ancestral_models_wide serves those).  An evaluation's index e is its index into loglik.
 *   node_sel: n_sel 1-based ape node ids in 1 .. n_tips + n_node, tips and duplicates allowed: the J = n_sel nodes to report, in
 *     that order.  NULL with n_sel = 0: every node in id order (J = n_tips + n_node).  A bad entry is PHM_ERR_BAD_INPUT naming
 *     its 0-based index; so are n_sel < 0 and n_sel > 0 with node_sel NULL.
 *   loglik: phm_loglik_models' values bit for bit.
 *   node_post: NULL, or [e][j][state], the state fastest: P(state of node j | tips_s, Q_k, pid_k), phm_expected_stats' node_post
 *     per model.
 *   joint_states: NULL, or [e][j]: the 1-based TRUE state of node j in the joint reconstruction, tips included (a missing tip
 *     and the hidden state behind an observe map come out reconstructed).
 *   joint_logp: NULL, or [e]: the log of that maximum (at most loglik); it needs joint_states.
 * node_post and joint_states both NULL is PHM_ERR_BAD_INPUT; the part not asked for is not computed and the other part is the
 * same bit for bit.  An evaluation whose log-likelihood is -inf gets NaN in node_post, 0 in joint_states and -inf in joint_logp;
 * it does not fail the call.  n_devices / devices[] shard the models and phm_debug_options.expect_chunk caps the chunks of
 * models, sites and level steps; neither changes an output bit.  phm_last_kernel_ms: device time of the call. */
int32_t phm_ancestral_models(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid,
                             int32_t n_pid, const int32_t* observe, const int32_t* site_of_model,
                             const int32_t* node_sel, int32_t n_sel, const phm_options* opt,
                             double* loglik, double* node_post, int32_t* joint_states, double* joint_logp);

/* ---- ancestral states of many rate matrices at 9..64 states ----
 * phm_ancestral_models' arguments, argument for argument, with the same meaning, output layouts, NULL rules and refusals, for
 * 9 <= n_states <= 64: amino acids, codons, hidden-rate models.  One state per lane, batched over models and sites; P_k(t_b) is
 * phm_expected_stats' (Pade(6) with its squaring counts).  loglik is phm_loglik_models' value and node_post is
 * phm_expected_stats' node_post of that model, both bit for bit; joint_states and joint_logp follow section 21's rules on the
 * device's own P (a back pointer is one byte).  2..8 states: PHM_ERR_UNSUPPORTED naming phm_ancestral_models; outside 2..64:
 * PHM_ERR_BAD_INPUT.  An evaluation whose log-likelihood is -inf, or whose model's Pade denominator met a zero pivot, gets
 * loglik = -inf, NaN in node_post, 0 in joint_states and -inf in joint_logp; it does not fail the call.  n_devices / devices[]
 * shard the models and phm_debug_options.expect_chunk caps the chunks of models, sites and level steps; neither changes an output
 * bit.  phm_last_kernel_ms: device time of the call. */
int32_t phm_ancestral_models_wide(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid,
                                  int32_t n_pid, const int32_t* observe, const int32_t* site_of_model,
                                  const int32_t* node_sel, int32_t n_sel, const phm_options* opt,
                                  double* loglik, double* node_post, int32_t* joint_states, double* joint_logp);

/* ---- forward simulation under many rate matrices in one call ----
 * K = n_models models (Q_k, pid_k), R = replicates histories each: one replicate dataset per posterior draw of the rates, R
 * bootstrap replicates under each of K fits, one dataset per prior draw.  H = K * R histories, history h = k * R + r, and history
 * h is -- in every state, count, tip, segment and segment dwell -- what phm_simulate_histories returns for GLOBAL replica
 * replica_offset + h under (Q_k, pid_k) with the same seed: only the Philox replica word carries h.  The per-history dwell sums
 * alone may differ from it in the last bits (they are accumulated in 64-bit fixed point, within 1e-12 * tree length of the
 * floating-point sums, and are the same bits whatever the chunks and devices are).
 *   Q: n x n x K, each matrix column-major, model slowest (phm_loglik_models' layout); pid: n x n_pid, n_pid = 1 (shared) or K,
 *     used as given (not normalised), as phm_simulate_histories uses it.
 *   tips: H x n_tips, history-major, 1-based reported states (through observe).  nodes: NULL, or H x (n_tips + n_node),
 *     history-major, 1-based true states by ape node id.  stats: H x (n + n*n + 1) column-major, phm_simulate_histories' columns.
 *   map_off NULL: no maps.  Otherwise the two-phase contract of phm_simulate_histories_maps with R = H, row h * n_edge + b.
 * Checked before any device call: the tree and edge lengths, every Q_k like phm_simulate_histories' Q and every pid column like
 * its pid (a bad model or pid column is named by its 0-based index), observe, the map arguments; PHM_ERR_BAD_INPUT for
 * replicates < 1, n_pid neither 1 nor K, reduce != 0 and replica_offset + H beyond the 32-bit replica word.  2 <= n <= 64.
 * phm_options.n_replicas is not read.  A branch that needs more than 9 999 jumps is PHM_ERR_CAPACITY naming the lowest-index
 * model that overflowed and an edge row of it; the loop is bounded, nothing faults.  n_devices / devices[] shard the models,
 * histories are chunked by free HBM and phm_debug_options.expect_chunk caps the histories per chunk (rounded up to 64) and the
 * edges per wave item; none of them changes an output bit.  phm_last_kernel_ms: device time of the call. */
int32_t phm_simulate_histories_models(const phm_tree* x, int32_t n_states, int32_t n_models, const double* Q, const double* pid,
                                      int32_t n_pid, const int32_t* observe, int32_t replicates, const phm_options* opt,
                                      int32_t* tips, int32_t* nodes, double* stats,
                                      int64_t* map_off, int64_t map_cap, double* map_dwell, int32_t* map_state);

/* ---- batched posterior sampling of the rates of an index model by exact data augmentation ----
 * n_chains chains in lock-step, one per lane.  The model: q_ij = theta_c for index[i, j] = c in 1..n_params, 0 for index 0 (index:
 * n x n column-major, diagonal ignored, every parameter owning at least one entry); the diagonal is minus the row's entries summed
 * left to right.  Prior: theta_c ~ Gamma(shape prior[.][c][0], rate prior[.][c][1]), n_prior = 1 (shared) or n_chains rows.
 * Iteration i of chain k: log p(tips | Q(theta)) (phm_loglik_models' value bit for bit), one exact history per site of the chain
 * -- bit for bit the history phm_sample_histories_models(draws = 1, replica_offset = i + opt->replica_offset, same seed) returns
 * for evaluation (site, chain k) among n_chains models -- and then theta_c ~ Gamma(shape + N_c, rate + W_c), N_c the history's
 * jumps over the entries of parameter c and W_c its dwell times, dwell_i once per entry (i, j) of c (sites ascending, entries
 * row-major).  A draw above theta_max (or not positive) is rejected and the old value kept, counted in rejected[chain][c].
 *   site_of_chain = n_chains site indices ("paired": chain k sees site site_of_chain[k] alone; sites may repeat), or NULL
 *     ("joint": every chain sees all S sites; log-likelihood and statistics are summed over the sites, ascending).
 *   theta0 [chain][n_params] in (0, theta_max]; theta_max truncates the prior and bounds the table of the sampler:
 *     (most rates in a row) * theta_max * (longest branch) above 32768 is PHM_ERR_UNSUPPORTED.
 *   rows = ceil(iters / thin); row r is iteration r * thin: theta [rows][chain][n_params] (row 0: theta0), loglik [rows][chain],
 *     stats NULL or [rows][chain][n + n(n-1)] (phm_expected_stats' columns: the history drawn under the row's theta).
 *   chain_status[chain]: 1 for a chain whose log-likelihood came out -inf; its rows are NaN from there on, the call goes on.
 * 2..8 states (more: PHM_ERR_UNSUPPORTED).  Bad index, prior, theta0, iters, thin or site: PHM_ERR_BAD_INPUT naming the chain or
 * parameter; the rest is checked as phm_loglik_models checks it; all before any device call.  Rate draws are addressed by
 * (parameter, chain, i + replica_offset): n_devices / devices[] (which shard the chains) and phm_debug_options.expect_chunk (which
 * caps the chunks of chains and branches) change no output bit.  phm_last_kernel_ms: device time of the call. */
int32_t phm_gibbs_rates(const phm_tree* x, int32_t n_states, const int32_t* index, int32_t n_params, int32_t n_chains,
                        const double* theta0, const double* prior, int32_t n_prior, double theta_max, const double* pid,
                        int32_t n_pid, const int32_t* observe, const int32_t* site_of_chain, int32_t iters, int32_t thin,
                        const phm_options* opt, double* theta, double* loglik, double* stats, int32_t* rejected,
                        int32_t* chain_status);

/* ---- host-side rate-matrix update of the Q-updating variants (no device needed) ----
 * One iteration of updatel01/l10 (bf) or updateksl01/l10, updaterkappas, updatelkappas, updategammas (ks) applied to Q
 * (column-major, edited in place) given a statistics row: n dwell sums then n*n counts, row-major (from,to). */
int32_t phm_qupdate_apply(int32_t variant, int32_t n_states, double* Q, double Omega, const double* prior, int32_t n_prior,
                          const double* row, uint64_t seed, uint32_t iter);

/* ---- inspection: the pruning kernel generated for an unstructured sparse chain matrix (no device needed) ----
 * 5..32 states, PHM_MAP_TILES: when the chain matrix (B, or B thresholded at 1e-7 for SPARSEmaketreelistMCMC, src/phylomap.cpp:801-816)
 * is at most half full and not banded, its pruning chains run in a kernel generated for the matrix's PATTERN and compiled at model
 * upload through hipRTC (what SPARSEmakePLrcpp :490-501 gets from sp_mat for any pattern).  This returns that kernel's HIP source for the
 * non-zero pattern of the n x n column-major matrix M: the number of bytes needed (including the terminator); up to `cap` bytes are
 * written to `buf` (may be NULL). */
int32_t phm_sparse_kernel_source(int32_t n_states, const double* M, char* buf, int32_t cap);

/* ---- host-side traversal orders (no device needed) ----
 * O(E) native replacement of the R helper preamble pruningwiseedgeorder / makenodelist / myreorder
 * (R/sumstatMCMC.R:1-18, interpreted O(E^2) loops around ape::reorder(x,"pruningwise")).
 * edge: n_edge x 2 column-major, 1-based.  nen: n_edge rows (1-based); nodelist: Nnode-1 node ids; root: node id. */
int32_t phm_tree_orders(int32_t n_tips, int32_t n_edge, const int32_t* edge, int32_t* nen, int32_t* nodelist,
                        int32_t* root);

/* ---- batched transition matrices (K1 / K1') ----
 * phm_expm_eigen: P_b = |L diag(exp(d_i t_b)) R|  (matexp, src/phylomap.cpp:2964-2968 + abs at :2980,:3042)
 * phm_expm_pade : P_b = expmat(Q t_b), Pade(6) scaling-and-squaring (arma::expmat call sites :3226,:3243,:3359,:3383)
 * out: n_t matrices, each n x n ROW-major (out[b*n*n + i*n + j]). */
int32_t phm_expm_eigen(int32_t n_states, const double* lefts, const double* rights, const double* d,
                       const double* t, int32_t n_t, int32_t device, double* out, double* kernel_ms);
/* phm_expm_eigen on the matrix cores (v_mfma_f64_16x16x4_f64), 16 < n_states <= 64: same product, fused k-slices, so the
 * last bits differ from phm_expm_eigen; the sumstatEXP sampler keeps the exact kernel. */
int32_t phm_expm_eigen_mfma(int32_t n_states, const double* lefts, const double* rights, const double* d,
                            const double* t, int32_t n_t, int32_t device, double* out, double* kernel_ms);
int32_t phm_expm_pade(int32_t n_states, const double* Q, const double* t, int32_t n_t, int32_t device,
                      double* out, double* kernel_ms);

/* phm_expm_pade with every matrix product on the matrix cores (v_mfma_f64_16x16x4_f64), 16 < n_states <= 64: solve(D, E) by
 * block Gauss-Jordan elimination without row exchanges between the 16 x 16 blocks; a matrix that meets a pivot below 1e-3 there
 * is recomputed by phm_expm_pade's pivoted kernel inside the same call.  Agrees with phm_expm_pade to rounding (<= 2e-13).
 * Test aid: phm_debug_options.pade_pivot_min overrides the 1e-3. */
int32_t phm_expm_pade_mfma(int32_t n_states, const double* Q, const double* t, int32_t n_t, int32_t device,
                           double* out, double* kernel_ms);

/* ---- resident engine (inputs stay in HBM between calls; what bench.py times) ---- */
int32_t phm_engine_create(const phm_tree* x, const phm_model* model, const phm_options* opt,
                          int32_t max_iters, phm_engine** out);
/* the same over a list of `n_trees` trees (equal tip and edge counts) sharing one model: opt->n_replicas chains PER TREE,
 * tree j's chains on their own 64-lane tiles (replica index j * n_replicas + c in every per-replica call; Philox replica
 * word replica_offset + 64 * tiles_per_tree * j + c).  reduce and tips_per_replica are not available here. */
int32_t phm_engine_create_multi(const phm_tree* trees, int32_t n_trees, const phm_model* model, const phm_options* opt,
                                int32_t max_iters, phm_engine** out);
/* enqueue iterations [iters_done, iters_done + n_iters) on `hip_stream` (a hipStream_t, NULL = default
 * stream); asynchronous */
int32_t phm_engine_run(phm_engine* e, int32_t n_iters, void* hip_stream);
/* wait for the stream, collect the device error word, fill timing */
int32_t phm_engine_sync(phm_engine* e);
/* copy statistics of iterations [iter0, iter0+n) to host.
 * reduce = 0: out[r][ (col)*n + (i-iter0) ] for replica r (n x cols column-major per replica)
 * reduce = 1: one n x cols column-major matrix (sum over replicas) */
int32_t phm_engine_read_stats(phm_engine* e, int32_t iter0, int32_t n, double* out);
/* reduce = 1 only: run the tile reduction on `hip_stream` and return a DEVICE pointer to n x cols doubles,
 * row-major [iteration][column] (for handing to RCCL without a host round trip).  The buffer belongs to this entry point
 * alone: it stays as the caller (or an in-place all-reduce) left it until the next phm_engine_reduced_stats_device call;
 * phm_engine_read_stats does not touch it */
int32_t phm_engine_reduced_stats_device(phm_engine* e, int32_t iter0, int32_t n, void* hip_stream, void** out_dev);
/* measurement aid: HIP-event time (ms) of n_iters repetitions of the pruning sweep alone (makePLrcpp*,
 * src/phylomap.cpp:503-529) on the current chain state; segment counts and paths are not modified */
int32_t phm_engine_time_pruning(phm_engine* e, int32_t n_iters, void* hip_stream, double* ms_out);
/* replace the rate matrix between sweeps (Q-updating variants, src/phylomap.cpp:1212-1217, :1862-1866); Q column-major,
 * B = I + Q/Omega recomputed, chain state kept; the bf/ks parameter columns record the Q in force at each sweep */
int32_t phm_engine_set_model(phm_engine* e, const double* Q);
/* chain state of one replica after the last iteration (tests): any pointer may be NULL.
 * seg_dwell: n_edge * seg_cap; node_states: 2*n_tips-1, 1-based; PL: (2*n_tips-1) x n row-major */
int32_t phm_engine_dump(phm_engine* e, int32_t replica, int32_t* seg_count, double* seg_dwell, int32_t seg_cap,
                        int32_t* node_states, double* PL);
int32_t phm_engine_info(phm_engine* e, phm_info* info);
/* measurement aid (phm_debug_options.phase_timing = 1, (tile, item) mappings): HIP-event milliseconds of the last phm_engine_run, summed over
 * its sweeps, for the four phases of a sweep: pruning levels (makePLrcpp*), root + node draws (sampleinternalnodes*), the branch
 * kernel (sampleabranch + updatedwelltimes), the statistics reductions.  Valid after phm_engine_sync. */
int32_t phm_engine_phase_ms(phm_engine* e, double* out4);
void    phm_engine_destroy(phm_engine* e);

#ifdef __cplusplus
}
#endif
#endif

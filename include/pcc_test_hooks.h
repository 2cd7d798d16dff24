/*
 * pcc_test_hooks.h -- TEST-ONLY entry points of libpcc_structural.so.  Not part of the product ABI
 * (pcc_structural.h / pcc_neighbour.h / pcc_emd.h): every function here is inert and returns 0 unless the
 * environment held PCC_TEST_HOOKS=1 when it was first called (tests/conftest.py sets it).
 */
#ifndef PCC_TEST_HOOKS_H
#define PCC_TEST_HOOKS_H

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* Make the next co-resident launch on the current device -- the cluster launch of pcc_auction_forward, resp. the
 * approximate EMD's resident launch of levels 0-2 (batch x tiles <= CUs) -- fail as if a sample barrier had timed out.
 * They exercise the one failure contract of pcc_emd.h and pcc_structural.h: the launch's outputs come out NaN for the
 * failed samples, and the next call of that kind on the device returns PCC_EINVAL ("did not complete") instead of
 * starting.  A call that runs no such launch (the batch, the sizes or a stream capture rule it out) leaves the request
 * pending.  Return 1 when armed. */
int pcc_test_inject_auction_failure(void);
int pcc_test_inject_approxmatch_failure(void);

/* A/B switches of the measurement scripts under tools/ and of the bit-identity tests (value 0 = the product's
 * behaviour).  They replace the PCC_* environment variables earlier rounds read inside the product library: nothing
 * in the product path selects behaviour from the environment any more.  Returns 1 when armed. */
enum {
    PCC_TUNE_SINKHORN_SPLIT = 0,   /* pcc_sinkhorn: S >= 1 = the columns of every scan in up to S slices (16 at the most, none shorter than a
                                      256-column tile); 0 = by n and m.  (Key 0: the last free slot of the table.) */
    PCC_TUNE_SW_PATH = 1,          /* pcc_sliced_wasserstein: 1..10 = the variant (threads, elements per thread) = (64,1) (64,2) (64,4) (128,4)
                                      (256,4) (512,4) (1024,4) (1024,8) (256,8) (512,8); a variant that cannot hold n is ignored.  (Key 1: a
                                      slot a retired switch left free.) */
    PCC_TUNE_AM_NOCULL = 2,        /* approxmatch: every exact-zero skip off (the no-skip roofline of bench.py) */
    PCC_TUNE_AM_NOSPLIT = 3,       /* approxmatch: everything on the caller's stream (no half-batch lanes) */
    PCC_TUNE_AM_NORESIDENT = 4,    /* approxmatch: levels 0-2 as one launch per pass even where the resident launch qualifies */
    PCC_TUNE_EDGE_SCATTER = 5,     /* gather / edge-feature backward: the per-edge ds_add_f32 scatter */
    PCC_TUNE_NBRSUM_SCATTER = 6,   /* neighbour-sum backward: the per-edge ds_add_f32 scatter */
    PCC_TUNE_AUCTION_CLUSTER = 7,  /* auction: value 1 = one workgroup per sample, 2..16 = that many per sample */
    PCC_TUNE_KNN_NOSPLIT = 8,      /* c >= 4 k-NN: 1 = the 128-query kernel everywhere, 2 = the role-split kernel everywhere */
    PCC_TUNE_KNN_WIDE = 9,         /* k-NN: 1 = every call through the wide path (knn_wide.hip), also where k <= 32, c <= 128 */
    PCC_TUNE_KNN_CROSS_SPLIT = 10, /* pcc_knn_cross: S >= 1 = the candidate axis in S slices (1 = one wave per query); 0 = by the row count */
    PCC_TUNE_FPS_PATH = 11,        /* pcc_fps: 1..6 = the register variant (block, P) = (64,4) (256,4) (256,8) (512,8) (1024,8) (1024,16), 7 = the
                                      memory path; a variant that cannot hold n is ignored */
    PCC_TUNE_OCCUPANCY_PATH = 12,  /* pcc_occupancy_grid: 1 = the global-atomic path everywhere, 2 = the LDS-histogram path (ignored where
                                      res^3 counters do not fit the workgroup's LDS, res > 32) */
    PCC_TUNE_BALL_PATH = 13,       /* pcc_ball_query: 1, 2 = candidates from global memory, 4 / 16 queries per workgroup; 3, 4 = candidates
                                      staged through LDS, 4 queries x tiles of 1024 / 16 queries x tiles of 4096 (the product's choice) */
    PCC_TUNE_GROUP_PATH = 14,      /* pcc_group_points / _bwd: 1 = the LDS path (ignored where not one channel row of n points fits a
                                      workgroup's LDS), 2 = the direct path (global gathers, global float atomics) */
    PCC_TUNE_INTERP_PATH = 15,     /* pcc_interpolate / _bwd, pcc_aggregate_points / _bwd (forward and grad_x) and
                                      pcc_kpconv_aggregate_bwd: 1 = the LDS path (ignored where not one channel row of n points fits a
                                      workgroup's LDS), 2 = the direct path (global gathers, global float atomics) */
    PCC_TUNE_KEYS = 16            /* keys are 0 .. PCC_TUNE_KEYS - 1 */
};
int pcc_test_set_tuning(int key, int value);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* PCC_TEST_HOOKS_H */

/*
 * armour_hip.h -- C ABI of libarmour_hip.so, the MI355X (gfx950) implementation of ARMOUR's
 * per-planning-iteration reachable-set + constraint pipeline.
 *
 * This is the drop-in boundary for the hot path of roahmlab/armour (RT/ =
 * kinova_src/kinova_simulator_interfaces/kinova_planner_realtime/).  The reference has no FFI for
 * this path: it spawns `armour_main` and exchanges text files (KSI/uarmtd_planner.m:158-219); its
 * only in-process native precedent is the MEX gateway of the robust controller
 * (MEXC/kinova_controller.cpp:19-84).  The entry points below are what a MEX / ctypes / cgo binding
 * of the planner would bind; each cites the reference interface it replaces.  INTEGRATION.md shows
 * the MEX stub and the file-protocol CLI built on them.
 *
 * Conventions: plain pointers and sizes; fp64; all host buffers caller-owned; the handle owns all
 * device memory; every function returns 0 on success or a negative ARMOUR_E* code and never
 * throws; armour_last_error() returns a thread-local message.  A handle is bound to one device and
 * one HIP stream; calls on different handles may run concurrently from different host threads.
 *
 * Batch semantics: a handle holds B independent planning problems (B >= 1) that share the robot,
 * the parameters and the obstacle count O.  B = 1 is the reference's use.  Arrays are
 * problem-major: q0[B][n], obstacles[B][O][12], k[B][n], g[B][m], jac[B][m][n].
 *
 * Constraint rows (RT/NLPclass.cu:46-49,117-164,304-320), m = n*T + J*T*O + 4n:
 *   [0, nT)                torque centre      g[t*n + j]
 *   [nT, nT + J*T*O)       collision          g[nT + (l*T + t)*O + o] = -max_p(...)  (feasible <= 0)
 *   then n rows min position, n rows max position, n rows min velocity, n rows max velocity.
 * Jacobian: dense, row-major values[row*n + col] exactly as IPOPT's `values` (RT/NLPclass.cu:348-357).
 */
#ifndef ARMOUR_HIP_H
#define ARMOUR_HIP_H

#include <stdint.h>
#include "armour_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ARMOUR_OK 0
#define ARMOUR_EINVAL (-1)    /* bad argument */
#define ARMOUR_EDEVICE (-2)   /* HIP runtime error (message has the hipError string) */
#define ARMOUR_ECAPACITY (-3) /* a polynomial zonotope outgrew its device table; raise the capacity in ArmourLimits */
#define ARMOUR_ESTATE (-4)    /* call order violated (e.g. eval before set_problems) */

typedef struct ArmourPlanner ArmourPlanner;

/* Device-table capacities (monomials). Zero fields take the defaults in parentheses. */
typedef struct ArmourLimits {
    int32_t max_batch;          /* problems per handle (1) */
    int32_t max_obstacles;      /* O upper bound (40, RT/Parameters.h:26 MAX_OBSTACLE_NUM; any value allowed) */
    int32_t link_monomials;     /* k-only monomials kept per link PZ (32) */
    int32_t torque_monomials;   /* k-only monomials kept per torque PZ (128) */
    int32_t work_monomials;     /* monomials of an intermediate PZ during FK/RNEA (1024) */
    int32_t raw_terms;          /* unsimplified terms of one PZ product (4096) */
} ArmourLimits;

/* ---- robot / parameter presets (RT/KinovaWithoutGripperInfo.h, RT/Parameters.h) ---- */
void armour_robot_kinova_gen3_no_gripper(ArmourRobot* robot);
void armour_robot_kinova_gen3_gripper(ArmourRobot* robot);   /* RT/KinovaInfo.h: 8 links, last joint fixed */
/* CMP/FetchInfo.h: 9 links (two fixed), 7 factors, joint axes {z,y,x,y,x,y,x}; link boxes and M_max are stand-ins
 * (include/armour_robot_fetch.h).  For payload-mass uncertainty set robot->mass_uncertainty_link[i] afterwards. */
void armour_robot_fetch(ArmourRobot* robot);
/* "Fetch 8-DOF" (BASELINE configs[4]): the arm above behind a torso yaw joint -- 9 links, 8 factors.  Filled by the 128-bit-key library only
 * (libarmour_hip_k128.so, armour_abi_max_factors() == 8); the 64-bit-key library returns ARMOUR_EINVAL (its key holds seven factors, as the
 * reference's: RT/PZsparse.h:8-21).  A derived preset, not reference data: include/armour_robot_fetch.h says what is assumed. */
int armour_robot_fetch8(ArmourRobot* robot);
void armour_params_default(ArmourParams* params, int32_t num_time_steps);

/* ---- lifetime ---- */
/* Replaces the process start-up of RT/armour_main.cu:11-86 (Obstacles ctor cudaMalloc x10, constant uploads).
 * `device` is a HIP device ordinal.  limits may be NULL. */
int armour_create(const ArmourRobot* robot, const ArmourParams* params, const ArmourLimits* limits,
                  int32_t device, ArmourPlanner** out);
void armour_destroy(ArmourPlanner* h);
const char* armour_last_error(void);
/* 1 if a HIP device is visible to this process, else 0 (never fails). */
int armour_device_available(void);

/* Optional page-locked host buffers for k / g / jac: armour_eval_g_jac DMAs straight into them instead of
 * staging through the runtime's bounce buffers (the reference pays 8-16 blocking cudaMemcpy per callback,
 * RT/CollisionChecking.cu:98-132). */
int armour_alloc_pinned(uint64_t bytes, void** out);
void armour_free_pinned(void* p);

/* ---- per-handle options ---- */
/* ARMOUR_OPT_P1_BUILD selects the reach-set build kernel of armour_set_problems* (value 0, 1 or 2):
 *   0  automatic (default): one wavefront per (problem, time step) for small batches, the time-vectorised kernel (one wavefront per
 *      50-64 time steps of a problem) from B*T >= 1550 on;
 *   1  always per time step;   2  always time-vectorised.
 * TOLERANCE CONTRACT.  Both kernels run the reference's operator sequence on the same operands and produce identical monomial keys,
 * coefficients and centres bit for bit; they add the pruned amounts of simplify() (RT/PZsparse.cu:327-341) into the independent
 * radii in a different order (per-lane partial sums + a wave reduction against a running sum in key order), so radii -- and through
 * them torque_radius, the link generators, g and jac -- may differ by rounding between the two: <= 1e-12 absolute on every table
 * and output, far inside the parity tolerances (tests/test_baseline_configs.py).  Within ONE kernel results are bit-reproducible
 * and independent of the batch mates and of the batch size.  A caller that needs bit-identical tables for the same problem across
 * batch sizes (or across the ranks of a sharded batch, whose shard sizes differ) sets option 1 (or 2) on every handle. */
#define ARMOUR_OPT_P1_BUILD 1
/* ARMOUR_OPT_P1_WORK_MEMORY_MB caps the device memory the time-vectorised build takes for its work slots, in MiB (0 = no cap, the
 * default: one block of ~112 MiB per compute unit while the batch has that many groups of time steps, 28.6 GiB for a batch of 128
 * problems on a 256-CU device).  With a cap the build runs on fewer blocks, which loop over the groups -- same tables bit for bit,
 * the build time grows with the rounds (a batch of 128 problems on half the blocks: about twice).  A cap below one block's slots
 * sends batches to the step-by-step kernel (a few GiB at most).
 * The work slots are ONE arena per device, shared by all handles of the process and held by a build only while it runs: two handles
 * building batches at the same time take turns on it (the kernel fills the device anyway), so they need it once, not twice. */
#define ARMOUR_OPT_P1_WORK_MEMORY_MB 2
/* ARMOUR_OPT_P1_KEEP_WORK_MEMORY (0 | 1, default 1): 1 leaves the device's shared work slots allocated between builds (they go with the
 * device's last handle); 0 releases them at the end of every armour_set_problems* of this handle, so that between builds the process
 * holds tables only.  Releasing costs the next large build its allocation: 0.6 ms of a 128-problem build's 10.4 ms as a rule, but
 * seconds now and then, when the runtime has to get 28.6 GiB back from the driver (measured) -- hence the default. */
#define ARMOUR_OPT_P1_KEEP_WORK_MEMORY 3

/* ---- launch-shape options (round 4: these were environment variables read once per process; two handles of one process can now
 * differ, and no stray variable changes a result).  Every one of them selects HOW the same operator sequence is laid out on the
 * device, never which operators run on which operands.  TOLERANCE CONTRACT of the whole group: monomial keys, coefficients and
 * centres of every table are bit-identical for every value; options marked (r) may change the ORDER in which pruned amounts are
 * added into the independent radii (<= 1e-12 on every table and output, as ARMOUR_OPT_P1_BUILD above); unmarked options leave
 * every bit alone.  Defaults are what bench.py and the tests measure; the values are tuning / test knobs. */
/* per-step reach-set kernel (p1_reach.hip: armour_p1_chain_kernel) */
#define ARMOUR_OPT_P1_STEP_WAVES 101          /* 0 automatic (default) | 1 | 3 | 4 wavefronts per (problem, time step) block */
#define ARMOUR_OPT_P1_STEP_FREE 102           /* 1 (default) free-running role waves | 0 a block barrier per joint */
#define ARMOUR_OPT_P1_STEP_SPLIT_FK 103       /* -1 automatic (default) | 0 | 1: forward kinematics as work items of their own */
#define ARMOUR_OPT_P1_STEP_AUX3 104           /* 1 (default) | 0: the w_aux recursion on the fourth wave of four-wave blocks */
#define ARMOUR_OPT_P1_MAX_WAVES_PER_CU 105    /* 1..8 (default 4): one-wave blocks resident per compute unit; the shipped kernels hold one wave per SIMD, so values above 4 act as 4 (they matter only in two-waves-per-SIMD development builds) */
#define ARMOUR_OPT_P1_TWO_PASS 106            /* 1 (default) | 0: large batches first with 2048-entry sort buffers, overflowing items rebuilt alone */
#define ARMOUR_OPT_P1_STEP_TAIL_CROSS 108     /* 0 off | n | 10 + n: four-wave blocks of a lone problem, w x (w_aux x com) of the last n <= 4 links built by the fourth (n) / the angular (10 + n) wave once its recursion is through */
#define ARMOUR_OPT_P1_STEP_QUEUE 109          /* 1 (default): the blocks draw their items from a counter, every problem's late time steps first | 2, 3: in index order, early steps first | 0: block k builds items k, k + blocks, ... */
#define ARMOUR_OPT_P1_STEP_PAIRS 107          /* 1 (default) | 0 | 2: four-wave blocks, backward pass -- the two idle waves join the recursion waves' operators (1: when every item has a block of its own; 2: always) */
#define ARMOUR_OPT_P1_STEP_TWO_CU 123         /* 3 (default) | 0 | 1 | 2: a lone problem's time step on TWO compute units -- a helper block per (problem, time step) reruns the two
                                                 angular-velocity recursions, builds the cross products that read nothing else (w x (w_aux x p), w x (w_aux x com), w_aux x (I w); level 3,
                                                 chains of at most 7 joints: R_t w_aux x (qd e) as well) and the step's forward kinematics, and hands the products over through the L2 of the
                                                 XCD the two blocks share (checked per item; otherwise, and whenever 2 T + 7 blocks do not fit the device, one CU per step as before).
                                                 Level 2: the main block drops its own w recursion; level 3: its w_aux recursion too.  Same tables bit for bit at every level.
                                                 10 + level, 20 + level: test hooks -- the helper agrees and hands over nothing (the build must notice and start again on one CU per step) /
                                                 the helper never says it has started (the main blocks give up after ~1.5 ms and build alone: good tables, late).  30 + level: the helper of an item is placed on
                                                 another XCD than its main block (every item must then decide against two CUs: one launch, good tables, no fall-back of the handle).  After either event the handle
                                                 stays on one CU per step and armour_get_option reads 0; setting the option again re-enables it */
#define ARMOUR_OPT_P1_STEP_LEAN_BACK 124      /* 1 (default) | 0 | 2 | 3: with a time step on two CUs at level 3 -- bit 0: the helper block also runs the backward pass's f-recursion (F_i handed over as the forward pass builds them, p x (R f) handed back), the main block's pair keeps R n and the four-term sum alone; bit 1 CLEAR: the JRS of the joints past the fourth is built by one wave of each block while the recursions run their first steps */
/* time-vectorised reach-set kernel (p1_tv.inc.h: armour_p1_tv_kernel) */
#define ARMOUR_OPT_P1_TV_MIN_GROUPS 110       /* default 31: automatic choice of ARMOUR_OPT_P1_BUILD takes this kernel from B*T >= 50 * value on */
#define ARMOUR_OPT_P1_TV_WAVES 111            /* 0 automatic (default) | 1 | 3 | 4 | 8 wavefronts per block (r: 4 and 8 share walks between waves) */
#define ARMOUR_OPT_P1_TV_FREE 112             /* 1 (default) | 0: free-running role waves | a block barrier per joint */
#define ARMOUR_OPT_P1_TV_SPLIT_FK 113         /* -1 automatic (default) | 0 | 1 */
#define ARMOUR_OPT_P1_TV_DEDICATED 114        /* 1 (default) | 0: eight-wave blocks may be chosen (development builds with two waves per SIMD only) */
#define ARMOUR_OPT_P1_TV_HELP_SHIFT 115       /* 0..3 (default 0): which helper wave serves which role wave in eight-wave blocks */
#define ARMOUR_OPT_P1_TV_HELPERS 116          /* (r) 0 every walk on its own wave | 1 (default) shared walks, the owner keeps 16/32 | 2..31: it keeps value/32 */
#define ARMOUR_OPT_P1_TV_HELP_MIN 117         /* (r) default 192: walks with fewer sorted terms stay on one wave */
#define ARMOUR_OPT_P1_TV_HELP_N 118           /* (r) 1 (default) | 0: the n-recursion shares its walks as well */
#define ARMOUR_OPT_P1_TV_AUX3 119             /* 1 (default) | 0: as ARMOUR_OPT_P1_STEP_AUX3 */
#define ARMOUR_OPT_P1_TV_TAIL_CROSS 121       /* as ARMOUR_OPT_P1_STEP_TAIL_CROSS, for the four-wave blocks of the time-vectorised kernel; default 111 since the end of round 6 (the cross product of the last link on the angular wave, every moment N on the F / N wave, which waited a fifth of the forward pass: B = 128 -1 %); + 100 (n + 1): the angular wave builds the moments of the last n links */
#define ARMOUR_OPT_P1_TV_ROW_WIDTH 122        /* 0 automatic (default) | 50 | 64: doubles per row of the kernel's work slots.  Automatic = 50 when a group of time steps fits (T = 100: two groups of 50; the rows are packed, -19 % of the build's L2-miss traffic), 64 otherwise; 50 with longer groups is refused.  Every bit of every table is the same for both. */
#define ARMOUR_OPT_P1_FULL_PLANES 120         /* 0 (default) the lean half-space table | 1 every plane and component resident (armour_get_hyperplanes builds it on demand otherwise) */
/* fused evaluation (p2_eval.hip) and its host entries (api.hip) */
#define ARMOUR_OPT_P2_EX 130                  /* 1 (default) | 0: the fixed-load-count kernels for problems with exactly 24 live planes */
#define ARMOUR_OPT_P2_NO_ZERO_TEST 134         /* 1 (default) | 0: EX launches whose problems have no live plane with a zero normal in any row (plane_zero of the build) take the kernels without the scan's zero-normal test; same rows bit for bit */
#define ARMOUR_OPT_STEPS_GRAPH_MIN 131        /* default 2: armour_eval_g_jac_device_steps submits >= this many steps as one graph; 0 never */
#define ARMOUR_OPT_CULL_ROWS 133              /* 0 (default) | 1: armour_eval_violations* evaluate the rows that can be violated for some k only (armour_get_row_relevance): same L1 violation, counts and verdict bit for bit; `worst` is the full evaluation's whenever a row is violated.
                                                * PRECONDITION: k inside [-1, 1]^n (the mask is a statement about the box).  armour_eval_violations (host k) takes every row when a component
                                                * lies outside; armour_eval_violations_device cannot look at k on the host: the record of a problem whose k is outside the box comes back
                                                * with feasible = -1 and worst_row = -2, and is to be re-evaluated with the option at 0 */
#define ARMOUR_OPT_PINNED_MODE 132            /* 0 (default) page-locked buffers through device staging + one DMA transfer | 1 the kernel reads / writes host memory itself */
/* armour_solve (solver.hip, solver_device.hip): iterates are bit-identical for every value (tests/test_solve.py) */
#define ARMOUR_OPT_SOLVE_SUB_TILES 140        /* default 48: row tiles per block aimed at when a batch is cut into sub-batches */
#define ARMOUR_OPT_SOLVE_DEVICE 141           /* 1 (default): the device-resident form (round 6: for every batch size; until round 5 from 2 problems on) | 0: never | 2: always */
#define ARMOUR_OPT_SOLVE_CUT_TILES 142        /* default 156: a batch whose blocks would walk more tiles each is cut */
#define ARMOUR_OPT_SOLVE_BLOCKS 143           /* 0 (default: as many as fit) | n: at most n blocks per problem */
#define ARMOUR_OPT_SOLVE_SUB_BATCH 144        /* 0 (default: by tiles) | n: sub-batches of at most n problems */
#define ARMOUR_OPT_SOLVE_ROW_CAP 145          /* 0 (default) | n: candidate-row buffers of n rows (tests: forces the overflow path) */
#define ARMOUR_OPT_SOLVE_HARD_CAP_S 146       /* 0 (default: from the time budget / iteration limit) | seconds: wall-clock cap of one persistent launch */
#define ARMOUR_OPT_SOLVE_WAVES_PER_SIMD 147   /* 0 automatic (default) | 1 | 2: register build of the persistent kernel */
#define ARMOUR_OPT_SOLVE_CULL 148              /* -1 automatic (default: from 150 000 collision rows in the batch on) | 0 | 1: the device-resident form walks only the rows that can pass
                                                * its candidate filter for some k (a second, wider mask than armour_get_row_relevance's: g_i + 2 |J_i|_1 can reach the bound); every
                                                * other row adds nothing the solver reads, so iterates and results are those of the full form bit for bit */
#define ARMOUR_OPT_FIRST_TUNING 101
#define ARMOUR_OPT_LAST_TUNING 148
/* bytes of device memory free / in all on `device` as the runtime reports them (hipMemGetInfo): what a caller sizes
 * ARMOUR_OPT_P1_WORK_MEMORY_MB against; either pointer may be NULL */
int armour_device_memory(int32_t device, uint64_t* free_bytes, uint64_t* total_bytes);
/* ARMOUR_MAX_FACTORS this library was built with: 7 (the shipped library: the reference's 64-bit monomial key, RT/PZsparse.h:8-21) or 8
 * (libarmour_hip_k128.so: 128-bit keys; every struct of armour_types.h that holds per-factor arrays is laid out for 8 there) */
int armour_abi_max_factors(void);
int armour_set_option(ArmourPlanner* h, int32_t option, double value);
/* armour_get_option: the current value of an option of this handle (status ARMOUR_EINVAL for an unknown option) */
int armour_get_option(ArmourPlanner* h, int32_t option, double* value);
/* Environment variables the library still reads (none of them changes a result): ARMOUR_P1_TRACE, ARMOUR_SOLVE_TIMING (one line of
 * timings per call on stderr), ARMOUR_WORKER_PARENT (armour_worker: exit with the parent process). */

/* ---- P1: reach-set build, once per planning iteration ---- */
/* Replaces RT/armour_main.cu:36-216 (parse armour.in, JRS, FK, RNEA x2, torque radius, half-space tables)
 * for B problems at once.  obstacles: [B][O][12], each = column-major Z=[c g1 g2 g3]
 * (KSI/uarmtd_planner.m:178; RT/CollisionChecking.cu:156-160).  Synchronous. */
int armour_set_problems(ArmourPlanner* h, int32_t B, int32_t O, const double* q0, const double* qd0,
                        const double* qdd0, const double* q_des, const double* obstacles);

/* armour_set_problems against MOVING obstacles: obstacle_frames is host [B][T][O][12] (T = num_time_steps), one zonotope per obstacle and plan
 * interval in the layout of armour_set_problems (centre, then 3 generators).  The half-space rows (l, t, .) -- the rows that say "link l's
 * occupancy over plan interval t does not meet the obstacle" -- are built from frame t instead of from one zonotope for every t; nothing else
 * of the build changes (reach sets, torque rows and limit rows do not read obstacles).
 * THE FRAME CONTRACT.  Plan interval t is the plan times [t D, (t + 1) D] with D = duration / T.  Frame t of problem b must cover everything
 * obstacle o can occupy at any time of that interval.  COVERING IS THE CALLER'S DUTY: the library takes a frame as given, exactly as it takes a
 * static obstacle as given, and its guarantee is the reference's per interval -- the link's occupancy over interval t does not meet frame t.
 * (armour_amd.worlds.moving_frames builds sound frames for axis-aligned boxes in linear motion.)
 * Arguments as armour_set_problems: a null obstacle_frames with O > 0 and non-finite entries are refused (ARMOUR_EINVAL), ArmourLimits.max_obstacles
 * means what it means there, and the handle stays usable after a refusal.  A table built from frames has no one centre per obstacle, so its d
 * column is stored at every batch size and the evaluations read it (a static batch of >= 8 problems recomputes d from the centres); the next
 * armour_set_problems on the handle restores the static forms, and the other way round.  Every consumer of the tables (evaluation, masks,
 * armour_solve*, armour_sweep, armour_eval_violations, armour_get_hyperplanes) works as after armour_set_problems.  Not available: the ARMTD
 * mode, armour_batch_* and the file protocol, whose obstacles stay static. */
int armour_set_problems_moving(ArmourPlanner* h, int32_t B, int32_t O, const double* q0, const double* qd0,
                               const double* qdd0, const double* q_des, const double* obstacle_frames);

/* ARMTD comparison mode: the same handle and the same callback surface for the reference's second
 * planner, kinova_planner_realtime_armtd_comparison ("CMP").  Replaces CMP/armtd_main.cu:36-216: constant-acceleration
 * trajectory q(t) = q0 + qd0 t + k t^2/2 (CMP/Trajectory.h:6-15), cos/sin JRS taken from the caller's offline tables and
 * rotated by q0 (CMP/Trajectory.cu:29-81), forward kinematics, half-space tables; no torque rows:
 * m = J*T*O + 4n (CMP/NLPclass.cu:42-43), collision rows first, then the joint-limit rows of the constant-acceleration
 * curve (CMP/Trajectory.cu:83-383).  After this call armour_get_sizes / get_bounds / eval_f / eval_grad_f / eval_g_jac* /
 * check_feasible / armour_solve and the table getters follow CMP/NLPclass.cu instead of RT/NLPclass.cu.
 *   jrs: [B][n][6][T], per joint the six rows armtd.in holds for it (KSI/uarmtd_planner.m:277-312): centre, k-generator
 *        and radius of cos(q - q0), then of sin(q - q0);  k_range: [B][n] (the number after each joint's rows, :314-315).
 * The ArmourParams of the handle supply T, the simplify threshold, the violation thresholds and the cost scale; its
 * k_range, duration and t_plan are not used in this mode. */
int armour_set_problems_armtd(ArmourPlanner* h, int32_t B, int32_t O, const double* q0, const double* qd0, const double* q_des,
                              const double* jrs, const double* k_range, const double* obstacles);

/* sizes after set_problems: n = NUM_FACTORS, m = constraint_number (RT/NLPclass.cu:46-49, get_nlp_info :62-82) */
int armour_get_sizes(const ArmourPlanner* h, int32_t* B, int32_t* n, int32_t* m);

/* ---- NLP callback surface (RT/NLPclass.h armtd_NLP : Ipopt::TNLP) ---- */
/* get_bounds_info, RT/NLPclass.cu:87-165.  x_l,x_u: [n] (shared by all problems); g_l,g_u: [B][m]. */
int armour_get_bounds(ArmourPlanner* h, double* x_l, double* x_u, double* g_l, double* g_u);
/* eval_f / eval_grad_f, RT/NLPclass.cu:207-267 (host arithmetic, 7 numbers).  k: [B][n]; f: [B]; grad_f: [B][n]. */
int armour_eval_f(ArmourPlanner* h, const double* k, double* f);
int armour_eval_grad_f(ArmourPlanner* h, const double* k, double* grad_f);
/* eval_g + eval_jac_g fused, RT/NLPclass.cu:272-396.  Host pointers; g and/or jac may be NULL.
 * Synchronous: H2D of k, one kernel launch, D2H of the requested outputs. */
int armour_eval_g_jac(ArmourPlanner* h, const double* k, double* g, double* jac);
/* Same, device-resident: d_k [B][n], d_g [B][m], d_jac [B][m][n] are device pointers on the handle's device
 * (d_g / d_jac may be NULL).  Enqueued on `stream` (a hipStream_t; NULL = the handle's own stream) and NOT
 * synchronised -- this is the entry the throughput benchmark and a device-side solver use. */
int armour_eval_g_jac_device(ArmourPlanner* h, const double* d_k, double* d_g, double* d_jac, void* stream);
/* `steps` consecutive fused evaluations enqueued back to back on `stream` without host synchronisation:
 * step s reads d_k + s*B*n (d_k holds [steps][B][n]) and overwrites d_g / d_jac.  One kernel launch per step
 * (the IPOPT iterate sequence of RT/armour_main.cu:273 with the solver's own arithmetic removed), executed in
 * order.
 * armour_prepare_steps(h, d_k, steps, d_g, d_jac) builds an instantiated hipGraph of those launches -- a chain of
 * `steps` kernel nodes -- without running it; later armour_eval_g_jac_device_steps calls with exactly these arguments
 * submit that graph (no host work per step) until the next armour_set_problems*.  The CONTENT of d_k may change
 * between calls, the pointers are part of the graph.  The four most recently used graphs are kept. */
int armour_eval_g_jac_device_steps(ArmourPlanner* h, const double* d_k, int32_t steps, double* d_g, double* d_jac,
                                   void* stream);
int armour_prepare_steps(ArmourPlanner* h, const double* d_k, int32_t steps, double* d_g, double* d_jac);
/* `points` evaluations of the SAME problems in ONE kernel launch: point s reads d_k + s*B*n and writes
 * d_g + s*B*m, d_jac + s*B*m*n (d_k [points][B][n], d_g [points][B][m], d_jac [points][B][m][n]; d_g / d_jac may be
 * NULL).  Every block keeps its share of the plane and PZ tables in registers across the points, so the tables are
 * read once per launch instead of once per point.  Results are bit-identical to `points` separate
 * armour_eval_g_jac_device calls.  For callers that know several trial points at once (line search, multi-start,
 * finite-difference checks -- the derivative checker of RT/armour_main.cu:248-251); IPOPT's own iterate sequence is
 * serial and uses the one-point entries above. */
int armour_eval_g_jac_device_multi(ArmourPlanner* h, const double* d_k, int32_t points, double* d_g, double* d_jac,
                                   void* stream);
/* finalize_solution feasibility re-check, RT/NLPclass.cu:422-538: feasible[b] = 1/0 from g[B][m] (host). */
int armour_check_feasible(ArmourPlanner* h, const double* g, int32_t* feasible);

/* ---- reduced outputs for throughput callers ---- */
/* A batch that evaluates 1e5 points/s cannot pull g and jac (2.29 MB per problem-evaluation at O = 50) over PCIe.  These entries run
 * the same fused kernel for g only, keep it on the device and hand back one record per problem: the row test of
 * armtd_NLP::finalize_solution (RT/NLPclass.cu:422-538; ARMTD mode: CMP/NLPclass.cu:391-402) applied on the device.
 *   l1_violation      sum over all rows of max(0, g_l - g, g - g_u)   (bounds of armour_get_bounds)
 *   worst, worst_row  the largest single-row violation and its row (lowest row among equals; -1 / 0.0 if no row is violated)
 *   n_violated        rows with a violation > 0
 *   n_outside_slack   rows finalize_solution rejects: torque rows beyond the bound by more than torque_violation_threshold, checked
 *                     collision rows above collision_violation_threshold, position / velocity rows outside their bounds
 *   feasible          n_outside_slack == 0: the verdict of armour_check_feasible on the same g
 * Sums run in a fixed order: the record depends on (problem, k) only, not on the batch or the device. */
typedef struct ArmourViolation {
    double l1_violation, worst;
    int32_t worst_row, n_violated, n_outside_slack, feasible;
} ArmourViolation;
/* d_k [B][n] and d_out [B] are device pointers; enqueued on `stream` (NULL = the handle's), not synchronised. */
int armour_eval_violations_device(ArmourPlanner* h, const double* d_k, ArmourViolation* d_out, void* stream);
/* host pointers, synchronous: 56 B in and 32 B out per problem instead of 8 m (1 + n) bytes */
int armour_eval_violations(ArmourPlanner* h, const double* k, ArmourViolation* out);
/* Row relevance of the current problem set -- the pruned constraint list of the reference's MATLAB path (KSI/uarmtd_planner.m:577-583: an
 * obstacle constraint is kept only if the forward occupancy can reach the buffered obstacle; :628-690: an input / limit constraint only if
 * `~(interval(...).sup < 0)`), which its C++ path does not have (RT/NLPclass.cu:272-396 evaluates every row at every iterate).
 * relevant[B][m] (row order of armour_eval_g_jac): 0 = the row cannot be violated for ANY k in [-1,1]^n -- a plane of its buffered obstacle
 * separates the whole family of sliced link centres (collision rows), the sliced torque's interval stays inside the bounds (torque rows) --
 * 1 otherwise; the 4n joint-limit rows are always 1.  Sound (a 0 is never violated: 1e-9 margin on the test), not tight.  On random worlds
 * about 2 % of the collision rows are 1.  n_relevant_collision_rows [B] and ms (device time of the test) may be NULL; so may `relevant`.
 * Computed once per problem set, on the device (relevance.hip).  ARMOUR_OPT_CULL_ROWS = 1 makes armour_eval_violations* use it.
 * THE RULE (normative; tests/relevance_rule.py restates it, tests/test_row_masks.py holds the kernels to it row by row).  c and coef_i: centre
 * and monomial coefficients of the row's link PZ; (A_p, d_p, delta_p): plane p of the row; sums in fp64.
 *   collision row:  L_p = |A_p . c - d_p| - (1 + 1e-12) sum_i |A_p . coef_i| - delta_p  over the LIVE planes p (armour_get_plane_skip) with a
 *                   non-zero normal; relevant = 0  iff  max_p L_p >= 1e-9.  (A zero-normal plane never separates, whatever its d and delta.)
 *   torque row:     cen and rad = sum_i |coef_i| of the row's torque PZ, bounds l, u:  relevant = 1  iff  cen + rad >= u - 1e-9  or
 *                   cen - rad <= l + 1e-9.
 *   limit rows:     always 1. */
int armour_get_row_relevance(ArmourPlanner* h, uint8_t* relevant, int32_t* n_relevant_collision_rows, double* ms);
/* The SOLVER's rows of the current problem set: solver_rows[B][m], 1 = the row can pass armour_solve's candidate filter for some k in [-1,1]^n
 * (g_i + 2 |J_i|_1 > u_i or g_i - 2 |J_i|_1 < l_i: solver_common.h; the filter leaves out rows that cannot become active within the variables'
 * box, and this mask the rows it leaves out at EVERY k) -- a superset of armour_get_row_relevance's mask; what the culled device form of armour_solve
 * walks (ARMOUR_OPT_SOLVE_CULL).  n_collision_rows [B] and n_torque_rows [B] may be NULL; so may `solver_rows`.
 * THE RULE (normative, in the terms of armour_get_row_relevance's).  deg_i = total degree of monomial i (the sum of its key's 2-bit fields).
 *   collision row:  solver_rows = 0  iff  relevant = 0  and some live plane p with a non-zero normal has
 *                       L_p - 3e-5 sum_i |A_p . coef_i|  >=  1e-9 + 2 |rd|_2 amax (1 + 3e-5) - u,
 *                   rd[e] = sum_i deg_i |coef_i[e]|;  amax = 1 for tables the library built (unit normals) and
 *                   max(1, max over the live planes p of |A_p|_2 (1 + 1e-12)) for tables loaded by armour_debug_load_tables.
 *   torque row:     solver_rows = 1  iff  relevant = 1  or the relevance test holds with (rad + 2 radd) (1 + 3e-5) in place of rad,
 *                   radd = sum_i deg_i |coef_i|.
 *   limit rows:     always 1.
 * (3e-5 > (1 + 1e-6)^21 - 1: the solver evaluates its lists at points up to 1e-6 outside the box, monomials have total degree <= 21.) */
int armour_get_solver_rows(ArmourPlanner* h, uint8_t* solver_rows, int32_t* n_collision_rows, int32_t* n_torque_rows, double* ms);

/* ---- in-process multi-device batch ---- */
/* One caller thread (MATLAB / MEX, a Python host) drives several GPUs: an ArmourBatch owns one ArmourPlanner per entry of `devices`
 * (an ordinal may repeat: two handles, two streams on one device).  B independent planning problems are dealt to the handles in
 * contiguous blocks -- device slot d owns problems [first[d], first[d+1]) with first[d] = d*(B/G) + min(d, B%G), the partition of
 * armour_amd/sharding.py -- and every call runs one host thread per slot, each driving its own handle and stream; the caller's
 * arrays are problem-major exactly as for a single handle and results are gathered in place.  There is no data-path collective and
 * no device-to-device traffic (problems share nothing).  The reference has no counterpart: it runs one problem per process
 * (RT/armour_main.cu); this is the in-process form of bench.py's one-rank-per-GPU sharding. */
typedef struct ArmourBatch ArmourBatch;
int armour_batch_partition(int32_t B, int32_t n_slots, int32_t* first /* [n_slots + 1] */);   /* pure host arithmetic (no GPU needed) */
int armour_batch_create(const ArmourRobot* robot, const ArmourParams* params, const ArmourLimits* limits,
                        const int32_t* devices, int32_t n_devices, ArmourBatch** out);
void armour_batch_destroy(ArmourBatch* bt);
int armour_batch_set_option(ArmourBatch* bt, int32_t option, double value);
int armour_batch_set_problems(ArmourBatch* bt, int32_t B, int32_t O, const double* q0, const double* qd0, const double* qdd0,
                              const double* q_des, const double* obstacles);
int armour_batch_get_sizes(const ArmourBatch* bt, int32_t* B, int32_t* n, int32_t* m, int32_t* n_slots);
int armour_batch_get_bounds(ArmourBatch* bt, double* x_l, double* x_u, double* g_l, double* g_u);
int armour_batch_eval_g_jac(ArmourBatch* bt, const double* k, double* g, double* jac);             /* full outputs (parity path) */
int armour_batch_eval_violations(ArmourBatch* bt, const double* k, ArmourViolation* out /* [B] */);  /* reduced outputs */
/* declared after ArmourSolveOptions below: armour_batch_solve */
/* armour_get_prune_margin of every problem of the batch: margin[B], problem-major like every other array */
int armour_batch_get_prune_margin(ArmourBatch* bt, double* margin /* [B] */);
/* ms of the slowest slot's last reach-set build (device time); per_slot may be NULL or [n_slots] */
int armour_batch_get_build_ms(ArmourBatch* bt, double* max_ms, double* per_slot);
/* armour_get_build_info of every slot: info[4 * slot + 0..3] (zeros for a slot without problems).  All slots of a problem set are built
 * by ONE kernel: with ARMOUR_OPT_P1_BUILD left automatic the one the smallest shard would take. */
int armour_batch_get_build_info(ArmourBatch* bt, int32_t* info /* [n_slots][4] */);

/* ---- caller side of the path: the trajectory the planner hands to the controller ---- */
/* uarmtd_planner.desired_trajectory, traj_type 'bernstein' (KSI/uarmtd_planner.m:846-925, with
 * PZM/utility/match_deg5_bernstein_coefficients.m and bernstein_to_poly.m): position / velocity / acceleration at time
 * t in [0, duration] of the degree-5 Bezier curve that starts at (q0, qd0, qdd0) and ends at rest at
 * q0 + k_range .* k -- the same curve the NLP constrains (RT/Trajectory.cu:542-602).  Stateless host arithmetic;
 * any of q / qd / qdd may be NULL.  The braking fallback (k = NaN: re-use the previous plan shifted by t_plan, or
 * hold position) is caller logic, see armour_amd/planner.py desired_trajectory. */
int armour_desired_trajectory(int32_t n, const double* q0, const double* qd0, const double* qdd0, const double* k_range,
                              double duration, const double* k, double t, double* q, double* qd, double* qdd);

/* ---- the tracking controller the planner's trajectories are executed with ---- */
/* kinova_controller(Kr, alpha, V_max, r_norm_threshold, q, qd, q_des, qd_des, qdd_des[, eps]) ->  [u, tau, v]
 * (kinova_robust_controllers_mex/kinova_controller.cpp:19-84; RobustController::update, ARMOUR method,
 * robust_controller.cpp:63-168) for B states at once: tau = nominal passivity-RNEA torque, the interval RNEA over
 * masses and inertias within +-model_uncertainty bounds the model error, v = robust input from the control barrier
 * condition on V = 1/2 r'M r <= V_max, u = tau - v.  One device thread per state.  All pointers are host pointers,
 * [B][n] row-major with n = robot->num_factors; Kr: [n] (diagonal gain).  ARMOUR_ESTATE if a nominal torque leaves its
 * interval (the reference throws).  ARMOUR_EINVAL, before the device is touched, for a non-finite entry of q .. qdd_des or Kr, a
 * non-finite alpha, V_max or r_norm_threshold, and a model_uncertainty that is negative or non-finite.  q_des - q is wrapped to
 * [-pi, pi) by the reference's loop up to 64 pi and by fmod first beyond: a bounded number of steps for every double. */
int armour_robust_controller(const ArmourRobot* robot, double model_uncertainty, const double* Kr, double alpha, double V_max,
                             double r_norm_threshold, int32_t B, const double* q, const double* qd, const double* q_des,
                             const double* qd_des, const double* qdd_des, double* u, double* tau, double* v);
/* Which of the controller's two kernels a call uses (the entry has no handle, so this is per process; bit-identical results
 * either way, tests/test_controller.py): -1 (default) the four-wave latency kernel up to 4096 states and one lane per state
 * beyond, 0 always one lane per state, 1 always the latency kernel. */
int armour_controller_set_kernel(int32_t which);
/* kinova_controller_ALTHOFF(Kr, Kp, Ki, maxError, q, qd, q_des, qd_des, qdd_des[, eps]) ->  [u, tau, v]
 * (kinova_robust_controllers_mex/kinova_controller_ALTHOFF.cpp:19-90; RobustController::update, ALTHOFF method,
 * robust_controller.cpp:63-128 -- the robust input of Giusti and Althoff, the controller kinova_compare_robust_controller.m runs beside
 * ARMOUR's) for B states at once: tau and the interval torque as in armour_robust_controller (the same nominal and interval passes,
 * without the interval M r pass), bound_i = max |interval torque_i - tau_i|, then
 *   phi_t = Kp[0] + Ki[0] e_acc[b],  kappa_t = Kp[1] + Ki[1] e_acc[b],  v = -(kappa_t |bound|_2 + phi_t) r,  u = tau - v
 * with r = (qd_des - qd) + Kr .* wrap(q_des - q).  No threshold on |r| and no division by it: r = 0 gives v = 0 and u = tau exactly.
 * e_acc [B] is the accumulated state error update() receives (NULL: zeros).  As the reference's MEX runs it e_acc is always 0 -- a fresh
 * controller per call and deltaT = 0, so ssErrorAccum never moves and maxError has no effect -- which is why maxError is no argument here.
 * One device lane per state, one kernel (no latency form: the study calls this with tens of thousands of states).  Pointers and shapes as
 * armour_robust_controller.  ARMOUR_EINVAL, before the device is touched, for a null argument (e_acc excepted), B < 1, a non-finite
 * entry of q .. qdd_des, Kr, Kp, Ki or e_acc, and a model_uncertainty that is negative or non-finite; ARMOUR_ESTATE if a nominal torque
 * leaves its interval; ARMOUR_EDEVICE without a device. */
int armour_althoff_controller(const ArmourRobot* robot, double model_uncertainty, const double* Kr, const double Kp[2], const double Ki[2],
                              const double* e_acc /* [B] or NULL = zeros */, int32_t B, const double* q, const double* qd, const double* q_des,
                              const double* qd_des, const double* qdd_des, double* u, double* tau, double* v);

/* ---- closed-loop tracking: the plan executed by an uncertain arm under the controller (tracking.hip) ---- */
/* uarmtd_agent.dynamics + uarmtd_agent.integrator with its low-level controller in the right-hand side (KSI/uarmtd_agent.m:280-293,
 * :360-405; KSI/uarmtd_robust_CBF_LLC.m:160-170) for B independent rollouts on the device, fp64 throughout.  Rollout b follows the
 * degree-5 Bezier reference of armour_desired_trajectory (q0[b], qd0[b], qdd0[b], end q0 + k_range .* k[b], `duration`) from t0 to t1.
 *   Integrator   classical RK4 on z = (q, qd), N = ceil((t1 - t0) / dt - 1e-9) steps of h = (t1 - t0) / N (not ode15s: a fixed
 *                step, so a rollout's bits depend on nothing but its own inputs); node k is at t0 + k h, node N at t1.
 *   Controller   ARMOUR_TRACK_CTL_ROBUST: RobustController::update, ARMOUR method, with opt->Kr .. model_uncertainty -- the arithmetic of
 *                armour_robust_controller;  _NOMINAL: u = the nominal passivity RNEA torque, v = 0 (KSI/uarmtd_nominal_passivity_LLC.m);
 *                _NONE: u = 0, the passive plant;  _ALTHOFF: RobustController::update, ALTHOFF method, with opt->Kr, model_uncertainty
 *                and Kp = opt->althoff_Kp -- the arithmetic of armour_althoff_controller with e_acc = 0 at every stage, as in the
 *                reference's runs; |v| goes into max_robust_input and status 1 means what it means under _ROBUST.  A non-finite
 *                althoff_Kp is ARMOUR_EINVAL under _ALTHOFF and ignored otherwise.
 *   Plant        qdd = M_true(q)^-1 (u - h_true(q, qd)), the controller's own nominal model (CoM frames) with link i's mass scaled by
 *                (1 + mass_scale[b][i]) and its CoM-frame inertia by (1 + inertia_scale[b][i]); M_true carries the armature on its diagonal
 *                (the reference's transmision_inertia), h_true = passivity RNEA (q, qd, qd, 0) with gravity.  Unlike uarmtd_agent, h_true
 *                includes the model's joint damping (zero on the Kinova presets).
 *   Monitors     at every node, from the first RK4 stage: |wrap(q_des - q)|, |qd_des - qd|, V_true = 1/2 r' M_true r
 *                (r = (qd_des - qd) + Kr .* wrap(q_des - q), the reference's true_V), |v|, |u_i| / torque_limits[i]; limit crossings as the
 *                reference's input_check / joint_limit_check (KSI/uarmtd_agent.m:517-590): |u_i| > torque_limits[i] (bit 0),
 *                q_i outside [state_limits_lb, state_limits_ub] (bit 1), |qd_i| > speed_limits[i] (bit 2).
 *   Stops        status 1: the robust update found the nominal torque outside the interval torque (the reference throws); status 2: a
 *                non-finite state.  The result then holds the state at the last node reached (t_end, steps).
 * Compare the maxima with the ultimate bound of the controller (KSI/uarmtd_robust_CBF_LLC.m:36-40):
 *   ub = sqrt(2 V_max / robot->M_min),  qe = ub / min(Kr)  (position),  qde = 2 ub  (velocity);  V stays <= V_max.
 * Work is chunked: every launch advances each live rollout by at most steps_per_launch steps and the host launches until all reach t1;
 * results are bit-identical for every steps_per_launch.  Arrays are host pointers, rollout-major: q0 / qd0 / qdd0 / k [B][n],
 * k_range [n], z0 [B][2n] (q then qd at t0; NULL: on the reference), mass_scale / inertia_scale [B][n] (NULL: zeros), results [B],
 * trace [B][N / record_every + 1][3n] (q, qd, u at nodes 0, r, 2r, ...; nodes after a stop are NaN; NULL or record_every = 0: none).
 * ms (may be NULL): device time of the whole call.  ARMOUR_EINVAL on bad arguments (checked before the device is touched). */
#define ARMOUR_TRACK_CTL_ROBUST 0
#define ARMOUR_TRACK_CTL_NOMINAL 1
#define ARMOUR_TRACK_CTL_NONE 2
/* (3 is unassigned and refused: callers and tests have relied on armour_track answering controller = 3 with ARMOUR_EINVAL since the entry
 * exists, so a new mode does not take the number) */
#define ARMOUR_TRACK_CTL_ALTHOFF 4
#define ARMOUR_TRACK_LIMIT_TORQUE 1
#define ARMOUR_TRACK_LIMIT_POSITION 2
#define ARMOUR_TRACK_LIMIT_SPEED 4
typedef struct ArmourTrackOptions {
    int32_t controller;        /* ARMOUR_TRACK_CTL_* */
    int32_t record_every;      /* trace every this many steps; 0 = no trace */
    int32_t steps_per_launch;  /* 0 = automatic (about 15 ms of device time per launch) */
    int32_t reserved0;
    double Kr[ARMOUR_MAX_FACTORS];
    double alpha, V_max, r_norm_threshold, model_uncertainty;   /* as armour_robust_controller */
    double dt, t0, t1, duration;                                /* 0 <= t0 < t1 <= duration; dt > 0 */
    double althoff_Kp[2];      /* _ALTHOFF: (phi, kappa) of v = -(kappa |bound| + phi) r; the first two of four doubles that were reserved */
    double reserved[2];
} ArmourTrackOptions;
/* What a result holds at the edges:
 *   - a torque limit <= 0 contributes no ratio to max_torque_ratio (nothing is divided by it) and still flags: ARMOUR_TRACK_LIMIT_TORQUE is
 *     set at the first node where that joint's u is not zero;
 *   - the maxima ignore NaN (fmax): a NaN candidate leaves a maximum as it was, an infinite one makes it infinite;
 *   - a status-2 rollout keeps the last finite state: q, qd and t_end are those of the node the failed step started from, `steps` is
 *     unchanged by it, that node's monitors (maxima, flags, first_violation_t) and its trace record are in, later trace records are NaN. */
typedef struct ArmourTrackResult {
    int32_t status;            /* 0 reached t1, 1 nominal torque outside the interval torque, 2 non-finite state */
    int32_t steps;             /* steps taken */
    int32_t limit_flags;       /* ARMOUR_TRACK_LIMIT_* crossed at some node */
    int32_t reserved;
    double t_end, q[ARMOUR_MAX_FACTORS], qd[ARMOUR_MAX_FACTORS];   /* the last node reached */
    double max_pos_error, max_vel_error, max_V, max_robust_input, max_torque_ratio;
    double first_violation_t;  /* the first node with a limit crossing; NaN: none */
} ArmourTrackResult;
/* Kr = robot->K on every joint, alpha = robot->alpha, V_max = robot->V_m, r_norm_threshold = 0, model_uncertainty = robot->mass_uncertainty
 * (KSI/uarmtd_robust_CBF_LLC.m:6-9 as the planner's robot constants set them), althoff_Kp = {28.1037, 28.1037} (:11), controller ROBUST, dt = 1e-3, t0 = 0, t1 = duration = 1,
 * no trace, automatic steps per launch. */
void armour_track_options_default(const ArmourRobot* robot, ArmourTrackOptions* opt);
int armour_track(const ArmourRobot* robot, const ArmourTrackOptions* opt, int32_t B, const double* q0, const double* qd0, const double* qdd0,
                 const double* k, const double* k_range, const double* z0, const double* mass_scale, const double* inertia_scale,
                 ArmourTrackResult* results, double* trace, double* ms);
/* the steps per launch armour_track takes for `controller` when opt->steps_per_launch = 0 (about 15 ms of device time per launch at the
 * per-step cost measured on the MI355X, tracking.hip); ARMOUR_EINVAL for an unknown controller */
int armour_track_auto_steps(int32_t controller);

/* ---- NLP solve of the planning iteration ---- */
/* Replaces IpoptApplication::OptimizeTNLP + armtd_NLP::finalize_solution (RT/armour_main.cu:237-304,
 * RT/NLPclass.cu:422-538) for all B problems of the handle at once: SQP on the device callbacks, start x = 0,
 * exact (constant, diagonal) cost Hessian, dense QP by a dual active-set method, L1-merit line search.
 * IPOPT itself is not part of this library; this solver returns a local optimum of the same NLP. */
typedef struct ArmourSolveOptions {
    int32_t max_iterations;   /* SQP iterations (60) */
    int32_t max_line_search;  /* halvings per iteration (12) */
    double tolerance;         /* step / violation tolerance (1e-4 = IPOPT_OPTIMIZATION_TOLERANCE, RT/Parameters.h:50) */
    double max_wall_time_s;   /* 0 = unlimited (reference: 0.5 s - t(P1) - 0.05 s, RT/armour_main.cu:227-229) */
    double force_host_qp;     /* which of the two forms of the solver runs -- both give the same iterates bit for bit:
                               *   0 (default) automatic: the whole SQP iterate in one persistent kernel (since round 6 for a lone problem too: the QP's
                               *     box-clipped first try -- armour_debug_qp_box -- settles the QPs of feasible problems without an active-set step, 0.07 ms
                               *     per solve on the reference's worlds; the host-driven form -- evaluations on the device, one launch each, the 7-variable
                               *     QPs on the host -- is 7 % faster on lone INFEASIBLE problems, which take hundreds of QP steps, and remains the fallback);
                               *   > 0: the host-QP form whatever the batch;   < 0: the persistent-kernel form whatever the batch. */
    double reserved[3];
} ArmourSolveOptions;
typedef struct ArmourSolveResult {
    double k_opt[ARMOUR_MAX_FACTORS];
    double cost;              /* eval_f at k_opt (includes COST_FUNCTION_OPTIMALITY_SCALE) */
    double max_violation;     /* L1 violation of g_l <= g <= g_u at k_opt */
    int32_t feasible;         /* finalize_solution verdict: what armour.out's "k_opt or -1" is decided on */
    int32_t iterations, evaluations;
    int32_t status;           /* 1 converged, 2 iteration limit, 3 inconsistent linearisation, 4 line search failed, 5 time limit */
    double time_ms;
} ArmourSolveResult;
void armour_solve_options_default(ArmourSolveOptions* opt);
int armour_solve(ArmourPlanner* h, const ArmourSolveOptions* opt, ArmourSolveResult* results /* [B] */);
int armour_batch_solve(ArmourBatch* bt, const ArmourSolveOptions* opt, ArmourSolveResult* results /* [B] */);
/* armour_solve from a start point of the caller's: k_start host [B][n], NULL = zeros (armour_solve(h, opt, r) IS armour_solve_from(h, opt, NULL, r)).
 * The reference starts at 0 and marks that as a weakness (RT/NLPclass.cu:193-198, "try to avoid local minimum"); its MATLAB path starts fmincon at a
 * random point.  Both forms of the solver take the start: the host-QP form and the persistent kernel, its culled variant included.
 *   - a component with |k_start| > 1 or a non-finite one: ARMOUR_EINVAL, before any HIP call (the variables' box; the culled form's row lists hold inside it);
 *   - NULL and an array of +0.0 give armour_solve's results bit for bit, in every field except time_ms;
 *   - the host form and the device form give bit-equal iterates from any start. */
int armour_solve_from(ArmourPlanner* h, const ArmourSolveOptions* opt, const double* k_start /* host [B][n]; NULL = zeros */,
                      ArmourSolveResult* results /* [B] */);

/* ---- candidate sweep: S trial points k of the SAME problems judged in one go (sweep.hip) ---- */
/* "Is there any safe plan in this reach set?"  The row test of armour_eval_violations and the cost of armour_eval_f for S candidates per problem,
 * on the relevant rows only (armour_get_row_relevance: the torque rows, the LISTED collision rows, the limit rows), and the best safe candidate
 * picked on the device.  What a caller does after an infeasible armour_solve: sweep, then armour_solve_from the winner (armour_amd/planner.py
 * solve_rescued).
 *   k_cand   host, [S][n] shared by all problems (per_problem = 0) or [B][S][n] (per_problem = 1); every |k| <= 1
 *   records  [B][S], may be NULL;  best [B], may be NULL;  ms = device time of the sweep's launches, may be NULL.  Synchronous.
 * CONTRACT
 *   Violation record.  records[b][s].v is the record armour_eval_violations gives for problem b at that k (ARMOUR_OPT_CULL_ROWS 0 or 1).  worst,
 *     worst_row, n_violated, n_outside_slack and feasible are EXACT: every row's g is computed with the fused evaluation's arithmetic in its own
 *     order (the arithmetic of p2_sparse.h's sparse_collision_row / sparse_torque_row and of the limit block, bezier.h / cacc.h).  l1_violation is
 *     within m * 2^-52 * l1 of that entry's value -- the bound of a sum of m non-negative terms taken in any order; the shipped kernel in fact
 *     keeps the layout of the row test (thread t of 256 owns the rows r = t mod 256 in ascending order, the same tree combines them), which
 *     gives the same bits.
 *   Independence.  A record depends on (problem, k) only: not on S, the candidate's position, the other candidates, B, or per_problem.
 *   Cost.  records[b][s].cost equals armour_eval_f at that k bit for bit (solver_common.h plan_point / wrap_to_pi, continuous joints first).
 *   Best candidate.  best[b] = the index of the candidate with the smallest cost among those with v.feasible == 1, the lowest index among equals;
 *     -1 if none is feasible.  Selected on the device.
 *   Arguments.  ARMOUR_EINVAL before the first HIP call if S < 1, S > 4096 (ARMOUR_SWEEP_MAX_CANDIDATES), or any |k| > 1 or non-finite k: the
 *     row lists hold inside the box only.
 *   Modes.  Every mode ARMOUR_OPT_CULL_ROWS = 1 supports: the Bezier trajectory, ARMTD comparison mode, and input_constraints_off (no torque rows).
 * Launches: two per call whatever S (the sweep; the selection), after the once-per-problem-set row lists.  A block serves one problem and a tile
 * of armour_sweep_tile() candidates: it reads each row's table entries once and evaluates them for the whole tile. */
#define ARMOUR_SWEEP_MAX_CANDIDATES 4096
typedef struct ArmourSweepRecord { ArmourViolation v; double cost; } ArmourSweepRecord;   /* 40 bytes */
int armour_sweep(ArmourPlanner* h, int32_t S, const double* k_cand, int32_t per_problem,
                 ArmourSweepRecord* records, int32_t* best, double* ms);
/* candidates per block of armour_sweep's kernel (a compile-time tile; tests take their S around it).  No result depends on it. */
int armour_sweep_tile(void);
/* test hook for the dense QP: min 1/2 x'diag(Gd)x + g0'x  s.t. lo <= A x <= hi (A row-major [m][n], n <= 7,
 * |bound| >= 1e18 = absent).  Host-only: runs without a GPU. */
int armour_debug_qp(int32_t n, const double* Gd, const double* g0, int32_t m, const double* A, const double* lo,
                    const double* hi, double* x, int32_t* feasible);

/* the same with the variables' box x_lo <= x <= x_hi appended as armour_solve appends it, and armour_solve's FIRST TRY (round 6): with a diagonal G the
 * minimiser over the box alone is the unconstrained one clipped variable by variable; when that point satisfies every row it is the QP's solution and
 * no active-set step is taken (steps = 0) -- on the reference's own worlds nearly every QP ends there.  first_try = 0: the active-set method alone.
 * Host-only.  steps / max_mult may be NULL. */
int armour_debug_qp_box(int32_t n, const double* Gd, const double* g0, int32_t m, const double* A, const double* lo, const double* hi,
                        const double* x_lo, const double* x_hi, int32_t first_try, double* x, int32_t* feasible, int32_t* steps, double* max_mult);

/* test hooks for the QP of one SQP step with its ELASTIC ATTEMPTS (sigma = 0, 0.5, 0.9, 0.99: a violated row may keep that fraction of its violation;
 * the first feasible attempt wins), posed as armour_solve poses it: n variables, the cost's diagonal Hd[n] > 0 and gradient gradf[n], the iterate x[n]
 * -- the box rows -1 - x <= d <= 1 - x are appended as the solver appends them -- and ncand <= 16384 candidate rows  a_i'd >= v_i - sigma max(v_i, 0)
 * (a: [ncand][n] row-major).  Both return the step d[n], feasible, the attempt taken (0..3; 3 with feasible = 0: none was feasible) and its largest
 * multiplier (max_mult may be NULL), and per attempt arrays of 4 ints (NULL: not wanted; -1: not reported).
 *
 * armour_debug_qp_elastic: the host form's code.  Host-only.  Per attempt tried: active-set steps, rows dropped from the active set, those of
 *   them that were not its last row, rows excluded, active rows at the end.
 * armour_debug_qp_device: the device form's QP (the persistent kernel's wave-level code, one attempt per wave) in a launch of its own: one block, no
 *   problem set.  wps: 1 | 2, the kernel build (waves per SIMD: ARMOUR_OPT_SOLVE_WAVES_PER_SIMD); lds_rows: candidate rows the LDS staging holds, 0 =
 *   what a solve of that build has (96 KB or 40 KB over 8 (ARMOUR_MAX_FACTORS + 1) bytes a row), or fewer (more: ARMOUR_EINVAL).  qp_iter: the steps
 *   of every attempt up to the one taken (the attempts above it may have been stopped early).  The two forms agree bit for bit. */
int armour_debug_qp_elastic(int32_t n, const double* Hd, const double* gradf, const double* x, int32_t ncand, const double* a, const double* v,
                            double* d, int32_t* feasible, int32_t* attempt, double* max_mult, int32_t* steps, int32_t* dropped,
                            int32_t* dropped_mid, int32_t* excluded, int32_t* active);
int armour_debug_qp_device(int32_t n, const double* Hd, const double* gradf, const double* x, int32_t ncand, const double* a, const double* v,
                           int32_t wps, int32_t lds_rows, double* d, int32_t* feasible, int32_t* attempt, double* max_mult, int32_t* qp_iter);

/* ---- diagnostics the reference writes to its 4 extra files (RT/armour_main.cu:329-372) ---- */
/* torque_radius [B][n][T]   (armour_control_input_radius.out holds its transpose) */
int armour_get_torque_radius(ArmourPlanner* h, double* torque_radius);
/* link_independent_generators [B][T][J][3][6] row-major (armour_joint_position_radius.out) */
int armour_get_link_generators(ArmourPlanner* h, double* gens);
/* sliced link centres at k: [B][T][J][3] (armour_joint_position_center.out; RT/NLPclass.cu:311-314) */
int armour_get_link_centers(ArmourPlanner* h, const double* k, double* centers);

/* ---- table introspection (parity tests, roofline accounting: SURVEY 8d Sigma M_link / Sigma M_torque) ---- */
/* which: 0 = links(l,t) 3x1, 1 = u_nom(j,t) 1x1.  Returns the monomial count (>= 0) or a negative error.
 * center (may be NULL) receives [2][sz]: the centre, then the independent (interval) radius.
 * keys/coeffs may be NULL; otherwise keys[count], coeffs[count][sz]. */
int armour_get_pz(ArmourPlanner* h, int32_t b, int32_t which, int32_t i, int32_t t, double* center,
                  uint64_t* keys, double* coeffs, int32_t capacity);
/* sum over all problems of monomial counts: out4 = {sum_link, sum_torque, max_link, max_torque} */
int armour_get_table_sizes(ArmourPlanner* h, int64_t* out4);
/* half-space tables in the reference's layout (RT/CollisionChecking.cu:215-227):
 * A [B][T][J][O][36][3], d and delta [B][T][J][O][36]; any pointer may be NULL. */
int armour_get_hyperplanes(ArmourPlanner* h, double* A, double* d, double* delta);
/* plane_skip [B]: bit p set = half-space p is redundant in EVERY collision row of the problem (zero normal, or bit for bit +- the
 * normal of an earlier plane of its row: RT/CollisionChecking.cu:252-259,268-279 can then neither take its value nor its normal), so
 * the table holds nothing for it and the fused evaluation does not read it.  With axis-aligned box obstacles 12 of the 36 planes.
 * For the byte accounting of bench.py (what one evaluation reads) and for tests. */
int armour_get_plane_skip(ArmourPlanner* h, uint64_t* plane_skip);
/* Prune margin of the last armour_set_problems*, per problem: margin[B] = the minimum over EVERY simplify() verdict of the build (RT/PZsparse.cu:305-316:
 * a summed monomial whose Frobenius norm is <= SIMPLIFY_THRESHOLD moves into the independent part, else it stays) of |norm - threshold| / threshold,
 * verdicts on an exactly zero norm left out -- how close the build came to a prune FLIP, where rounding of the last bits decides whether a monomial
 * of norm ~5e-4 is kept as a monomial or folded into the radius: a legitimate change of g by up to that norm, and of the key sets.  Every stated
 * tolerance of this library against the reference's arithmetic (tests/: identical key sets, 1e-11 on tables, 1e-9 / 1e-8 on g / jac) holds while no
 * verdict came closer than ~1e-9; the reference cannot tell (it does not record it), the CPU oracle can (oracle_min_margin), and with
 * this entry so can a production call: both reach-set kernels keep, per lane, the smallest distance of a verdict's squared norm to the squared
 * threshold (two instructions per verdict) and reduce it per problem.  Two conventions differ from the oracle's figure, neither where it matters:
 * which side of the threshold the nearest verdict fell on is not recorded and the kept side's figure is reported -- below the other side's by a
 * relative O(margin) -- and a verdict on an exactly zero norm (a lane of the time-vectorised build without that monomial) counts with the margin
 * sqrt(2) - 1, so 0.414 is the largest value reported while any exists.  1e300 for a problem without a verdict.  Cost: profiles/r06_prune_margin.txt.
 * ARMOUR_ESTATE after armour_debug_load_tables. */
int armour_get_prune_margin(ArmourPlanner* h, double* margin /* [B] */);
/* ms spent in the last armour_set_problems (device time, hipEvent) */
int armour_get_build_ms(ArmourPlanner* h, double* ms);
/* how the last armour_set_problems built its tables: out4 = {kernel that produced them (ARMOUR_P1_KERNEL_*), waves per block of
 * its last launch, sort-buffer entries per wave of that launch, launches of reach-set kernels in all}.  A launch whose sort buffers or
 * slot pools overflow is repeated with the next block shape (and a time-vectorised build that cannot be helped that way is repeated
 * step by step), so `launches` > 1 tells a caller that the limits in ArmourLimits are too small for the fast path; tools and tests
 * read the kernel.  {0,0,0,0} after armour_debug_load_tables. */
#define ARMOUR_P1_KERNEL_PER_STEP 1
#define ARMOUR_P1_KERNEL_TIME_VECTORISED 2
int armour_get_build_info(ArmourPlanner* h, int32_t* out4);
/* name of the P2 kernel as it appears in rocprofv3 kernel traces */
const char* armour_p2_kernel_name(void);

/* ---- test hook: one wave-level polynomial-zonotope operator on caller-supplied operands ---- */
/* Runs the device implementation of one operator of RT/PZsparse.cu (the same functions the reach-set kernel uses):
 *   op 0 mul 3x3*3x1, 1 mul 3x3*3x3, 2 mul 1x1*1x1, 3 mul 1x1*3x1 (:864-994); 4 a+b, 5 a-b on 3x1 (:743-834);
 *   6 addOneDimPZ(a 3x1, b 1x1, r) (:1068-1085); 7 stack(a,b,c) (:1087-1116); 8 cross(a, const), 9 cross(const, a),
 *   10 cross(a, b) (:1118-1167); 11 consts[0]*a + consts[1]*b on 1x1 (:996-1030 + :743-764);
 * and the compound operators of the reach-set chain, each the composition named with simplify() after every step:
 *   12 sum3 = (a + b) + c on 3x1, with r >= 0: c is 1x1 and goes into entry r (addOneDimPZ), r = -1: c is 3x1;  13 sum4 = ((a + b) + c) + d on 3x1;
 *   14 comb3 = (consts[0]*a + consts[1]*b) + consts[2]*c on 1x1;  15 embedOneDim = addOneDimPZ(PZsparse(0,0,0), a 1x1, r);
 *   16 (a + cross(w, consts)) + c on 3x1, operands a, w, c;  17 transpose of a 3x3 (:1050-1066, no simplify).
 * Operand o: sz[o] entries per coefficient (row-major) -- 1, 3 or 9 as the op code's operator takes them, anything else is ARMOUR_EINVAL --,
 * cnt[o] monomials with keys[o][cnt] sorted unique and coef[o][cnt][sz]; cen / ind / ind2 are [nops][9]; nops <= 4.  A key is passed in the
 * library's own width: sizeof(pzkey_t) / 8 u64 words, low word first -- one word in the 7-factor ABI, two in the 8-factor (128-bit key) ABI of
 * include/armour_types.h --, in keys[o] and in out_keys alike.
 * cap_key, cap_raw: the entries of the wave's two sort buffers (keys | term indices): 0, 0 = both as wide as the handle's raw-term limit; otherwise
 * powers of two in [64, 8192] -- the builds give the fourth wave of a four-wave block 1024 / 2048 and every wave of the 128-bit ABI cap / 2 keys,
 * and the sorter an operator takes depends on the two separately.
 * Result: out_keys[<=out_cap], out_coef[<=out_cap][sz],
 * out_misc[64] = {count, sz, error flags, cen[9], ind[9], ind2[9], [30] the operator's shader-clock cycles, [31] raw terms,
 * [32..] phase counters in -DP1_PROFILE builds, [60] the smallest |s - [61]| over the SQUARED norms s of the operator's simplify() verdicts,
 * [61] the squared threshold they were compared with (+inf in [60]: no verdict; armour_get_prune_margin)}. */
int armour_debug_pz_op(ArmourPlanner* h, int32_t op, int32_t nops, const int32_t* sz, const int32_t* cnt, const uint64_t* const* keys,
                       const double* const* coef, const double* cen, const double* ind, const double* ind2, const double* consts,
                       int32_t r, int32_t out_cap, uint64_t* out_keys, double* out_coef, double* out_misc, int32_t cap_key, int32_t cap_raw);

/* ---- test hook: load externally built reach-set tables instead of running P1 ---- */
/* Used only by tests to isolate P2 (tables built by the CPU oracle); never called by the product path.
 * link_* : [B][J][T] counts, centers [..][2][3] (centre, independent radius), keys [..][cap_l], coeffs [..][cap_l][3]
 * torque_*: [B][n][T] counts, centers [..][2], keys [..][cap_t], coeffs [..][cap_t]
 * A,d,delta in the reference layout (see armour_get_hyperplanes); torque_radius [B][n][T]. */
int armour_debug_load_tables(ArmourPlanner* h, int32_t B, int32_t O, const double* q0, const double* qd0,
                             const double* qdd0, const double* q_des, const int32_t* link_count,
                             const double* link_center, const uint64_t* link_keys, const double* link_coeffs,
                             int32_t cap_l, const int32_t* torque_count, const double* torque_center,
                             const uint64_t* torque_keys, const double* torque_coeffs, int32_t cap_t,
                             const double* A, const double* d, const double* delta, const double* torque_radius);

/* ---- test hook: the row LISTS behind armour_get_row_relevance (which = 0) / armour_get_solver_rows (which = 1) ---- */
/* Read only: copies out what relevance.hip built for the current problem set and launches nothing.  ARMOUR_ESTATE without a problem set, and
 * when the set's lists have not been built yet (call armour_get_row_relevance / armour_get_solver_rows first).  Every pointer may be NULL.
 *   rows       [B][Q]   problem b's listed collision rows q, ascending, in rows[b][0 .. count[b])  (entries behind the count are not defined)
 *   count      [B]
 *   aux, aux_count      which = 0: the same rows by residue class of the row index, aux [B][256][ceil(Q / 256)]: class c holds the listed q
 *                       with (row0 + q) mod 256 == c, ascending, aux_count [B][256] of them;
 *                       which = 1: the torque rows of the solver's mask, aux [B][row0] ascending, aux_count [B]
 *   pack_off   [2 B]    [2 b] the first double of problem b's block of packed plane entries, [2 b + 1] its row stride = count[b] rounded up to 16
 *   packed              the packed block: entry [(j * 5 + c) * stride + i] of problem b's block = component c of {Ax, Ay, Az, d, delta} of the
 *                       j-th live plane (ascending; armour_get_plane_skip) of listed row i.  packed_total (may be NULL) receives its length in
 *                       doubles; with `packed` given, packed_capacity < that length is ARMOUR_EINVAL. */
int armour_debug_get_row_lists(ArmourPlanner* h, int32_t which, int32_t* rows, int32_t* count, int32_t* aux, int32_t* aux_count,
                               int64_t* pack_off, double* packed, int64_t packed_capacity, int64_t* packed_total);

/* ---- test hooks: which fused-evaluation kernel a one-point launch takes, and the plane-table addressing its launch plan carries ---- */
/* armour_debug_p2_plan: the plan of a one-point armour_eval_g_jac_device launch of the handle's current problem set.
 *   verdict [6]   {d recomputed from the obstacle centres, at most 24 live planes per problem (6-slot kernels), the exact-layout (EX) kernel,
 *                  bytes of kernel arguments, every problem shares problem 0's live-plane mask, the mask travels by value}
 *   fields [20]   what an EX launch reads instead of deriving it per block, all 0 when it is not one; in bytes from the start of one problem's
 *                 plane table: {one plane of a paired section, section CD, section DLL, section D, the whole table, the link x link records},
 *                 then, when the mask is shared, p * (bytes of a plane) of the six planes of wave 0 and of wave 1, and p - 21 of the first
 *                 link x link plane of wave 2 and of wave 3 (0 otherwise: the kernel walks the mask).
 * armour_debug_p2_plan_shape (host only, no handle, no device): the same for tables of B problems with T steps, J links, n factors, O obstacles,
 * capL stored and max_link live monomials per link PZ and the live-plane masks skip [B] (bit p set: plane p is skipped); recompute_d != 0:
 * tables without the d column.  A shape whose per-problem tables reach 2^32 bytes is no EX launch (verdict[2] = 0). */
int armour_debug_p2_plan(ArmourPlanner* h, int32_t* verdict, uint32_t* fields);
int armour_debug_p2_plan_shape(int32_t B, int32_t T, int32_t J, int32_t n, int32_t O, int32_t capL, int32_t max_link, int32_t recompute_d,
                               const uint64_t* skip, int32_t* verdict, uint32_t* fields);
/* armour_debug_p2_zero_plan: does that launch take the EX kernel WITHOUT the scan's zero-normal test (*nonzero = 1), and the two masks [B] the
 * verdict rests on: skip (armour_get_plane_skip) and zero -- bit p set: plane p has a normal with three components == 0.0 (so -0.0 counts) in at
 * least one row of the problem; bits of skipped planes carry no meaning; all ones when the masks are not a build's (loaded tables).  The verdict
 * is on only for an EX launch with zero[b] & ~skip[b] empty for every problem and ARMOUR_OPT_P2_NO_ZERO_TEST = 1.
 * armour_debug_p2_zero_plan_shape (host only, no handle, no device): the plan of armour_debug_p2_plan_shape's table shape with the masks skip [B]
 * and zero [B]; verdict [2] = {the exact-layout (EX) kernel, the one without the zero-normal test}. */
int armour_debug_p2_zero_plan(ArmourPlanner* h, int32_t* nonzero, uint64_t* skip, uint64_t* zero);
int armour_debug_p2_zero_plan_shape(int32_t B, int32_t T, int32_t J, int32_t n, int32_t O, int32_t capL, int32_t max_link, int32_t recompute_d,
                                    const uint64_t* skip, const uint64_t* zero, int32_t* verdict);

/* ---- test hooks: the block steps under the per-world planner kernels (armour_tree_plan, armour_path_shortcut, armour_ik, armour_ws_tree_plan) ---- */
/* armour_debug_block_steps: ONE block of 256 lanes runs each cooperative step once on the caller's per-lane values (all [256]) and touches no
 * planner state.  Lane t holds the key (d[t], v[t]) -- a lane without a key passes (+inf, INT32_MAX) --, the flag flag[t] != 0 and the term n[t].
 *   min_d, min_v  the smallest key in the order "d, then v"
 *   first         the smallest lane with its flag set, INT32_MAX when there is none;   any   1 when some lane has it set, else 0
 *   sums [256]    sums[t] = n[0] + ... + n[t];   total = sums[255]
 * ARMOUR_EINVAL on a null pointer, ARMOUR_EDEVICE without a device.
 * armour_debug_block_split (host only): how `items` >= 1 work items share the 256 lanes when each is tested against O obstacles:
 * split [256][4] = {G, per, o0, o1} of lane t -- G = min(O, 256 / items) lanes to an item when allowed != 0, 2 items <= 256 and O > 1, else 1;
 * per = 256 / G items at a time; lane t is lane g = t mod G of item t / G and takes the obstacles [o0, o1) = [g O / G, (g + 1) O / G).
 * armour_debug_block_owner (host only): end [n] ascending, n <= 256, end[k] = one past the last work item of candidate k;
 * owner[i] = the number of ends <= item[i] = the first candidate whose end exceeds item[i], n when there is none. */
int armour_debug_block_steps(const double* d, const int32_t* v, const int32_t* flag, const int32_t* n, double* min_d, int32_t* min_v, int32_t* first,
                             int32_t* any, int32_t* sums, int32_t* total);
int armour_debug_block_split(int32_t items, int32_t O, int32_t allowed, int32_t* split);
int armour_debug_block_owner(const int32_t* end, int32_t n, int32_t count, const int32_t* item, int32_t* owner);

/* ---- roadmap high-level planner: a joint-space roadmap checked against worlds' obstacles on the device ---- */
/* What the reference's sample-based HLP does with its prebuilt collision_checker (kinova_samplebased_HLP_realtime): node feasibility,
 * node clearance and the collision-free subset of a roadmap's edges, per world; then a search of the free graph for waypoints.
 *
 * Geometry.  Link l (all num_joints links, fixed trailing ones included) at configuration q is the box
 *   p_l(q) + R_l(q) (c_l + diag(h_l) beta),  |beta|_inf <= 1,
 * c_l = link_zonotope_center[l], h_l = link_zonotope_generators[l], and the frames of armour_amd/robot_geometry.py link_frames:
 *   p_l = p_{l-1} + R_{l-1} trans_l,  R_l = R_{l-1} rpy(rots_l) Rot(axes_l, q_l)   (Rot = identity on a fixed joint).
 * An obstacle is the usual 12 numbers Z = [c g1 g2 g3].
 *
 * Node rule (exact).  For a (link, obstacle) pair, d = (p_l + R_l c_l) - c, the 6 generators are g1..g3 and h_lk u_k (u_k = column k
 * of R_l), and the 15 plane normals are the cross products of generator pairs (RT/CollisionChecking.cu polytope_PH, applied to a static
 * box).  For a normal m from the pair (a, b), with the other four generators "rest":
 *   value(m) = (|m.d| - sum over rest of |m.g|) / |m|          (positive: this plane separates the two)
 * A link x link pair's normal is the third axis u_k itself (R_l is a rotation), its value |u_k.d| - sum_a |u_k.g_a| - h_lk.
 * A normal is DEGENERATE and skipped when |m|^2 <= 1e-18 |a|^2 |b|^2 (the sine of the pair's angle <= 1e-9; for an obstacle x link
 * pair |u_k| = 1 is used): it is rounding noise, or zero for a zero generator.  A zonotope's facets in 3-D are spanned by generator
 * pairs, so the test is exact up to the facets of the skipped, nearly parallel pairs (a sliver of relative width <= 1e-9).
 *   pair clearance = max over the used planes of value;  node clearance = min over (link, obstacle) of pair clearance
 *   (+inf with no obstacle).  The node is FREE iff its clearance > 0.  This is -link_c of the reference (there link_c <= 0 is safe).
 * A node's verdict does not depend on the order of links or obstacles.
 *
 * Edge rule (conservative).  Edge (a, b) is the joint-space segment q(t) = a + t D, t in [0, 1], D = b - a, wrapped on continuous
 * joints: D_j = d - 2 pi floor((d + pi) / (2 pi)), d = b_j - a_j.  It is cut into S = max(1, ceil(max_j |D_j| / edge_step))
 * sub-segments; sub-segment s is checked at its midpoint q(t_s), t_s = (2s + 1) / (2S), with every half-size of link l enlarged by
 *   r_l = (sum over actuated j <= l of rho_{j,l} |D_j|) / (2S),   rho_{j,l} = sum_{i=j+1..l} |trans_i| + |c_l| + |h_l|.
 * rho_{j,l} bounds the distance from joint j's origin p_j to any point of link l's box, for every configuration (triangle inequality
 * along the chain).  Soundness: inside sub-segment s every joint is within |D_j|/(2S) of its midpoint value.  Moving the joints there
 * one at a time, turning joint j by theta turns every point of link l >= j about an axis through p_j, which moves it by at most
 * rho_{j,l} theta; so every point of link l anywhere on the sub-segment is within r_l of the midpoint box, i.e. inside the box with
 * half-sizes h_l + r_l.  The edge is FREE iff every enlarged box of every sub-segment is separated (value > 0) from every obstacle,
 * so no configuration on a free edge collides, and a free edge has free endpoints.
 *
 * Device.  armour_roadmap_check runs ONE launch for W worlds: a work item is (world, node) or (world, edge sub-segment); the
 * sub-segment offsets depend only on the roadmap, robot and edge_step and are built at create time.  fp64 throughout.
 * Handles are not thread-safe; calls on one handle are synchronous. */
typedef struct ArmourRoadmap ArmourRoadmap;
#define ARMOUR_ROADMAP_MAX_OBSTACLES 256   /* 216 B of LDS each: 55 KB per block at the cap */
/* nodes [N][n] (n = robot->num_factors), edges [E][2] node indices, continuous [n] (1 = wrapped; NULL: robot->continuous),
 * edge_step > 0 in radians.  ARMOUR_EINVAL on a bad argument, ARMOUR_ECAPACITY when N + (edge sub-segments) exceeds 2^31 - 1. */
int armour_roadmap_create(const ArmourRobot* robot, int32_t N, const double* nodes, int32_t E, const int32_t* edges,
                          const uint8_t* continuous, double edge_step, int32_t device, ArmourRoadmap** out);
void armour_roadmap_destroy(ArmourRoadmap* rm);
/* N, E and the total number of edge sub-segments (any pointer may be NULL) */
int armour_roadmap_get_sizes(const ArmourRoadmap* rm, int32_t* N, int32_t* E, int64_t* edge_samples);
/* obstacles [W][O][12], O <= ARMOUR_ROADMAP_MAX_OBSTACLES (pad worlds with fewer boxes with far-away ones).  Outputs, each may be NULL:
 * node_free [W][N] (0/1), edge_free [W][E] (0/1), node_clearance [W][N] (computed only when requested), ms = device time of the
 * launch.  The handle keeps every world's verdicts and obstacles for armour_roadmap_plan. */
int armour_roadmap_check(ArmourRoadmap* rm, int32_t W, int32_t O, const double* obstacles, uint8_t* node_free, uint8_t* edge_free,
                         double* node_clearance, double* ms);
/* armour_roadmap_check against obstacles in LINEAR MOTION, over a time window per world.  obstacles [W][O][12] is every obstacle's pose at
 * world time 0, velocity [W][O][3] its constant velocity, t_from / t_to [W] the window of world w in world time (t_from <= t_to).
 * Window rule.  The host computes once per world mid[w] = 0.5 * (t_from[w] + t_to[w]) and half[w] = 0.5 * (t_to[w] - t_from[w]) and hands
 *   these two numbers to the kernel, so host and device judge by the same doubles.  A node is FREE in the window when the node rule's pair
 *   tests pass with, for obstacle o, the box centre x - v_o mid (component-wise x[i] - v[i] * mid) and every half-size h_l + |v_o|_2 half
 *   (|v_o|_2 = sqrt((v0^2 + v1^2) + v2^2), computed once per obstacle when it is staged); its clearance is the minimum of those pair
 *   values.  An edge is FREE when every sub-segment of the edge rule passes the same tests with the half-sizes h_l + (r_l + |v_o|_2 half).
 *   Sub-segment counts and offsets are the static check's (armour_roadmap_get_sizes stays valid).
 * Soundness.  Within [t_from, t_to] obstacle o leaves its pose of time mid by at most |v_o| half.  A meets B + d exactly when A - d meets B,
 *   and a box whose half-sizes grow by rho contains the box (+) a ball of radius rho.  So no configuration on a free node or edge meets an
 *   obstacle at ANY time of the window, whatever the time at which the arm passes it (the static argument supplies r_l).
 * With zero velocities the masks and clearances are armour_roadmap_check's bit for bit, for any window (x - 0 * mid = x,
 *   h + (r + 0 * half) = h + r); t_from == t_to is the verdict at an instant.
 * State.  The handle keeps the obstacles, velocities and windows: until the next check, armour_roadmap_plan, armour_roadmap_descend,
 *   armour_roadmap_connect_batch, armour_roadmap_descend_batch and the seeds of armour_roadmap_field test the edges that join a point to the
 *   roadmap by the window rule of the point's world.  armour_roadmap_check returns the handle to the static rule.  Either check ends the
 *   field.  armour_roadmap_knn and the self masks read masks only.
 * Device.  One launch for all W worlds; RM_OBS_STRIDE + 4 doubles of LDS per obstacle (248 B: 62 KB per block at the cap).
 * ARMOUR_EINVAL before a device is touched: armour_roadmap_check's refusals; a null or non-finite velocity, t_from or t_to;
 * t_from[w] > t_to[w]. */
int armour_roadmap_check_moving(ArmourRoadmap* rm, int32_t W, int32_t O, const double* obstacles, const double* velocity,
                                const double* t_from, const double* t_to, uint8_t* node_free, uint8_t* edge_free,
                                double* node_clearance, double* ms);
/* the same rule by the same functions in a host loop, for a handle of armour_roadmap_create_host (any other: ARMOUR_EINVAL); runs without
 * a GPU.  It leaves the host state of the device entry -- W, O, the masks, the staged obstacles and the windows -- so armour_roadmap_plan
 * works on that handle afterwards. */
int armour_roadmap_check_moving_host(ArmourRoadmap* rm, int32_t W, int32_t O, const double* obstacles, const double* velocity,
                                     const double* t_from, const double* t_to, uint8_t* node_free, uint8_t* edge_free,
                                     double* node_clearance);
/* Host search over world w of the last check: the direct start -> goal edge if it is free; else start and goal are joined to their
 * connect_k nearest free nodes (wrapped joint distance) by edges checked with the edge rule, and A* runs over the free edges with
 * wrapped-distance weights.  path [max_points][n] = start, nodes..., goal; *points = 0 when there is no path.  ARMOUR_ESTATE before
 * a check; ARMOUR_ECAPACITY (with *points = the length needed) when max_points is too small. */
int armour_roadmap_plan(ArmourRoadmap* rm, int32_t w, const double* q_start, const double* q_goal, int32_t connect_k,
                        int32_t max_points, double* path, int32_t* points);

/* Cost-to-go fields (roadmap_field.hip): in a trial a world's goal never changes, so the shortest free-graph distance from EVERY node to
 * the goal, with a successor pointer, is computed once for all W worlds of the last check, in one launch.
 *
 * Graph of world w: the roadmap's edges e with edge_free[w][e]; with armour_roadmap_use_self on, also self_edge_free[e] (free in both
 *   masks, as armour_roadmap_plan).  A free edge has free endpoints, so node masks are not needed.
 * Edge length: len[e] = wrapped distance of nodes[a] -> nodes[b], a = edges[2e], b = edges[2e + 1] (the square root of the sum over
 *   joints, in order, of the squared wrapped difference), evaluated once on the host; the device takes no square root.
 * Seeds: the goal of world w is joined to its connect_k nearest free nodes by host-checked edges, exactly as armour_roadmap_plan joins
 *   its goal; such a node i starts at seed[i] = wrapped distance of goal -> node i (every other node: seed = +inf).
 * Field: cost[w][.] is the GREATEST solution of  cost[v] = min(seed[v], min over free edges (u, v) of fl(cost[u] + len[e])),
 *   +inf where no seed is reachable.  Every sum is one fp64 add, accumulated from the goal outwards.
 * Successor: next[w][v] = -1 when cost[v] is infinite; ARMOUR_ROADMAP_NEXT_GOAL when seed[v] == cost[v]; otherwise the smallest u over
 *   the free edges at v with fl(cost[u] + len[e]) == cost[v] and cost[u] < cost[v].  With every length above half an ulp of the costs
 *   (any roadmap of distinct nodes at a sensible spacing) the second condition follows from the first.  It is there for edges that join
 *   equal costs -- length 0 (a self loop, duplicate nodes) or a length the sum absorbs -- where each end would name the other: the costs
 *   fall strictly along next[], so a walk never cycles.  Limitation: a node that reaches its cost ONLY over such an edge has next = -1
 *   although its cost is finite, and armour_roadmap_descend through it is ARMOUR_ESTATE.
 * Determinism: x -> fl(x + len) is monotone and never decreases x, so the greatest solution is unique; any relaxation order, in place
 *   or not, ends at the same doubles, and so does a heap Dijkstra from the seeds.  The device's result is defined bit for bit.
 * Device: one block per world sweeps its cost row in place until a sweep changes nothing (at most N + 1 sweeps, else ARMOUR_ESTATE);
 *   W = 1 therefore runs on one compute unit. */
#define ARMOUR_ROADMAP_NEXT_GOAL (-2)
/* goals [W][n] for the W worlds of the last armour_roadmap_check.  Outputs, each may be NULL: cost [W][N] (+inf unreachable),
 * next [W][N], reached [W] (nodes with a finite cost), sweeps [W], ms (device time of the launch).  The handle keeps goals,
 * cost and next on the host for armour_roadmap_descend.  ARMOUR_ESTATE before a check (or, with self masks on, before a self check). */
int armour_roadmap_field(ArmourRoadmap* rm, const double* goals, int32_t connect_k, double* cost, int32_t* next,
                         int32_t* reached, int32_t* sweeps, double* ms);
/* Host, no search: the direct start -> goal edge if free (as armour_roadmap_plan); else among start's connect_k nearest free nodes
 * whose connecting edge is free and whose cost is finite, the one with the smallest fl(distance + cost) (first in nearest order on a
 * tie), then next[] to the goal.  path = start, nodes..., goal; *points = 0: no path; *length = that smallest sum (0-point: +inf;
 * direct edge: the wrapped distance; may be NULL).  A walk longer than N + 1 steps is ARMOUR_ESTATE.  armour_roadmap_check,
 * armour_roadmap_check_self and armour_roadmap_use_self each end the field: ARMOUR_ESTATE until the next armour_roadmap_field.
 * ARMOUR_ECAPACITY (with *points = the length needed) when max_points is too small. */
int armour_roadmap_descend(ArmourRoadmap* rm, int32_t w, const double* q_start, int32_t connect_k, int32_t max_points,
                           double* path, int32_t* points, double* length);

/* Nearest-neighbour search over the handle's nodes (roadmap_knn.hip): Q queries in one call, brute force on the device.
 *
 * Distance of a query q and a node x: the roadmap's wrapped distance.  Joint by joint in index order, D_j = the wrapped difference of
 *   the edge rule on continuous joints and x_j - q_j otherwise; acc += D_j * D_j from 0; d = sqrt(acc).  fp64, no fused multiply-add.
 * Candidates of query i: the nodes v with
 *   mask_row[i] < 0 (or mask_row == NULL), or v free in world mask_row[i] of the last armour_roadmap_check -- node_free[w][v], ANDed
 *     with the self mask self_node_free[v] when armour_roadmap_use_self is on (what the search entries take as free);
 *   v != exclude[i] (exclude may be NULL; an entry that names no node, e.g. -1, excludes nothing);
 *   d <= radius (radius = +inf: no limit).
 * Result of query i: the first min(k, #candidates) candidates in the TOTAL order (d, v) ascending -- distance first, then the smaller
 *   index: index[i][0..count[i]), dist[i][..], the rest of the k slots padded with -1 / +inf.  A total order makes the result unique,
 *   so it does not depend on how the nodes are dealt to lanes, waves and blocks or on the order partial lists are merged in: the device
 *   and the host entry return the same bits.  It is the order armour_roadmap_plan / _field / _descend join a start or goal by
 *   (std::partial_sort of (distance, index) over the free nodes).
 * Arguments: 1 <= k <= ARMOUR_ROADMAP_KNN_MAX, else ARMOUR_EINVAL; Q < 0, a non-finite query, a negative or NaN radius: ARMOUR_EINVAL.
 *   Q = 0 or N = 0: ARMOUR_OK, nothing written.  A mask_row entry >= 0 before a check (or, with the self masks on, before a self
 *   check) is ARMOUR_ESTATE, one >= W ARMOUR_EINVAL.  *ms (may be NULL): device time of the launches.
 * Device: Q >= ARMOUR_ROADMAP_KNN_MANY queries take one lane per query (the nodes cut into up to 16 slices when the queries alone do
 *   not fill the device); fewer take one block per (query, 256 nodes).  Every shape writes sorted partial lists and a second launch
 *   merges them by rank.  DESIGN.md 4.12b.
 * armour_roadmap_knn_host is the same rule in a host loop and touches no device; a handle of armour_roadmap_create_host serves it,
 * armour_roadmap_check_moving_host and armour_roadmap_plan after that check (and nothing that needs the device: those entries return
 * ARMOUR_EDEVICE on it). */
#define ARMOUR_ROADMAP_KNN_MAX 64
#define ARMOUR_ROADMAP_KNN_MANY 2048
int armour_roadmap_create_host(const ArmourRobot* robot, int32_t N, const double* nodes, int32_t E, const int32_t* edges,
                               const uint8_t* continuous, double edge_step, ArmourRoadmap** out);
int armour_roadmap_knn(ArmourRoadmap* rm, int32_t Q, const double* queries, const int32_t* mask_row, const int32_t* exclude,
                       int32_t k, double radius, int32_t* index, double* dist, int32_t* count, double* ms);
int armour_roadmap_knn_host(ArmourRoadmap* rm, int32_t Q, const double* queries, const int32_t* mask_row, const int32_t* exclude,
                            int32_t k, double radius, int32_t* index, double* dist, int32_t* count, double* ms);
/* Q queries joined to the graph in one call: for query i the connect_k (0..ARMOUR_ROADMAP_KNN_MAX) nearest free nodes of world
 * world[i] by the search above (node / dist [Q][connect_k], -1 / +inf padded, count [Q]) and, on the device in the same call, the edge
 * rule q[i] -> node for each (edge_ok [Q][connect_k], 0 in the padding) and, with target ([Q][n], may be NULL), q[i] -> target[i]
 * (direct [Q]).  With the self masks on an edge must pass the self edge rule too, as everywhere.  This is what the search entries
 * compute when they join a start or a goal, before they drop the nodes whose edge is not free.  State rules: armour_roadmap_plan's. */
int armour_roadmap_connect_batch(ArmourRoadmap* rm, int32_t Q, const int32_t* world, const double* q, const double* target,
                                 int32_t connect_k, int32_t* node, double* dist, uint8_t* edge_ok, int32_t* count, uint8_t* direct,
                                 double* ms);
/* armour_roadmap_descend for Q queries (world[i], q_start[i]) with ONE armour_roadmap_connect_batch call (target = each world's field
 * goal); the choice among the joined nodes and the walk along next[] are armour_roadmap_descend's own code.  status[i]: 0 no path,
 * 1 the direct edge, 2 through the nodes seq[seq_off[i] .. seq_off[i + 1]) (node indices; the path is start, those nodes, the goal);
 * length[i] as armour_roadmap_descend (may be NULL).  seq_off [Q + 1] is always complete: ARMOUR_ECAPACITY when seq_off[Q] exceeds
 * seq_capacity (then seq is not written).  State and argument rules: armour_roadmap_descend's, connect_k <= ARMOUR_ROADMAP_KNN_MAX. */
int armour_roadmap_descend_batch(ArmourRoadmap* rm, int32_t Q, const int32_t* world, const double* q_start, int32_t connect_k,
                                 int32_t seq_capacity, int32_t* seq_off, int32_t* seq, uint8_t* status, double* length);

/* Time slices (roadmap_slices.hip): the window rule of armour_roadmap_check_moving on K consecutive windows of every world's clock in ONE
 * launch, and an earliest-arrival search over (node, slice) states on the result.  DESIGN.md 4.16a.
 *
 * Slices.  The boundaries of world w are t_k = t0[w] + (double)k * dt, k = 0..K, computed once on the host and returned in slice_times
 *   [W][K + 1].  Slice k is the window [t_k, t_k+1]; the host computes mid_k = 0.5 * (t_k + t_k+1) and half_k = 0.5 * (t_k+1 - t_k) from those
 *   doubles and hands [W][K] of each to the kernel, so the device, the host twin and armour_roadmap_check_moving on
 *   (slice_times[w][k], slice_times[w][k + 1]) judge by the same numbers.
 * Outputs, each may be NULL.  Bit k of node_slices[w][v] is node_free[w][v] of armour_roadmap_check_moving on slice k, bit k of
 *   edge_slices[w][e] is edge_free[w][e] on it; bits >= K are 0.  There is no clearance.  Extra edge i (Q of them; Q = 0 with null arrays
 *   is allowed) joins extra_a[i] to extra_b[i] ([Q][n]) in world extra_world[i] and is judged by the edge rule with the handle's edge_step:
 *   extra_slices[i].  a == b gives S = 1 and r = 0, the node rule on that configuration.  *ms: device time of the launches.
 * State.  The handle keeps the slice tables with their W, O, K, dt and t0 as state of their own, on the device (and on the host when both
 *   node_slices and edge_slices were asked for); the last check's masks, obstacles, windows and field are not touched, so
 *   armour_roadmap_plan and armour_roadmap_descend answer after a sliced check as before it.  The self masks are not read.
 * Device.  A block serves one world (obstacles, mid and half in LDS: 248 B per obstacle + 16 B per slice, 63 KB at both caps); a lane is a
 *   node, an edge sub-segment or an extra sub-segment, walks its links once and keeps the slices still free in a 64-bit mask.
 * ARMOUR_EINVAL before a device is touched: armour_roadmap_check_moving's refusals (t0 in place of the windows); K < 1 or
 *   K > ARMOUR_ROADMAP_SLICES_MAX; dt not finite or <= 0, or a last boundary that is not finite; Q < 0 or a null extra array with Q > 0; an
 *   extra_world outside [0, W); an extra configuration that is not finite.
 * armour_roadmap_check_slices_host: the same function in a host loop, for a handle of armour_roadmap_create_host (any other: ARMOUR_EINVAL). */
#define ARMOUR_ROADMAP_SLICES_MAX 64
int armour_roadmap_check_slices(ArmourRoadmap* rm, int32_t W, int32_t O, const double* obstacles, const double* velocity,
                                const double* t0, double dt, int32_t K, int32_t Q, const int32_t* extra_world, const double* extra_a,
                                const double* extra_b, uint64_t* node_slices, uint64_t* edge_slices, uint64_t* extra_slices,
                                double* slice_times, double* ms);
int armour_roadmap_check_slices_host(ArmourRoadmap* rm, int32_t W, int32_t O, const double* obstacles, const double* velocity,
                                     const double* t0, double dt, int32_t K, int32_t Q, const int32_t* extra_world, const double* extra_a,
                                     const double* extra_b, uint64_t* node_slices, uint64_t* edge_slices, uint64_t* extra_slices,
                                     double* slice_times);
/* Earliest arrival over the slice tables of the last armour_roadmap_check_slices, all W worlds in one launch.
 *
 * Graph of world w: the roadmap's N nodes with mask node_slices[w][v]; node N, the start, with mask start_mask[w] | 1 (the arm is where it
 *   is in slice 0); node N + 1, the goal, with mask goal_mask[w]; the roadmap's edges with edge_slices[w][e]; and the world's extra edges
 *   (x_u, x_v, x_len, x_mask)[i], X in all, sorted by x_world, ends in [0, N + 2).  Only the low K bits of a mask given here are read.
 * Steps: steps(len) = max(1, ceil(len / step_len)), step_len in radians (nominal speed x dt), evaluated on the host for the roadmap's edge
 *   lengths (armour_roadmap_field's len[e]) and for x_len; the device sees int32.  An edge with steps > K is unusable.
 * Operators on 64-bit masks (no implementation shifts by 64): avail(m, c) = AND over i < c of (m >> i) -- every slice of a traversal is free;
 *   fill(x, m) = the least y that holds x & m with ((y << 1) & m) inside y -- waiting at a node while it stays free.
 * reach [W][N + 2] is the LEAST family of masks with reach[N] holding fill(1, start_mask | 1), every reach[v] closed under fill(., mask[v]),
 *   and for every usable edge (u, v) of c steps and mask m, in both directions, reach[v] holding ((reach[u] & avail(m, c)) << c) & mask[v].
 *   All operators are monotone on a finite lattice: the least fixed point is unique and any in-place sweep order ends at it.  A move
 *   advances the slice, so sweeps that close the waits end within K + 1 sweeps; more is ARMOUR_ESTATE.
 * goal_slice[w]: the lowest set bit of reach[N + 1], -1 if none.
 * Path: the backward walk from (N + 1, goal_slice).  At (v, k), v != N: the first usable incident edge with c <= k and bit k - c set in
 *   reach[u] and in avail(m, c) -- the roadmap's edges in row order (neighbour ascending, then edge id), then the world's extras in list
 *   order -- leads to (u, k - c); else (v, k - 1), a wait.  The walk stops at node N.  path_node / path_slice [W][64] list the visits from the
 *   start onward, path_len[w] of them (0: no path), -1 behind them: a node with the slice at which it is reached, the start with the slice at
 *   which the path leaves it.  Waits are implicit; slices increase strictly, so 64 entries suffice.
 * Every output may be NULL.  ARMOUR_ESTATE before a sliced check, and while armour_roadmap_use_self is on: the self masks are not part of
 *   the space-time search.  ARMOUR_EINVAL: step_len not finite or <= 0, extras not sorted by world or out of range, a negative or
 *   non-finite x_len.  armour_roadmap_arrival_host: the same functions world after world on the host, for a handle of
 *   armour_roadmap_create_host after armour_roadmap_check_slices_host; reach, goal_slice and the paths are the device's, sweeps may differ. */
int armour_roadmap_arrival(ArmourRoadmap* rm, double step_len, int32_t X, const int32_t* x_world, const int32_t* x_u, const int32_t* x_v,
                           const double* x_len, const uint64_t* x_mask, const uint64_t* start_mask, const uint64_t* goal_mask,
                           uint64_t* reach, int32_t* goal_slice, int32_t* path_len, int32_t* path_node, int32_t* path_slice,
                           int32_t* sweeps, double* ms);
int armour_roadmap_arrival_host(ArmourRoadmap* rm, double step_len, int32_t X, const int32_t* x_world, const int32_t* x_u, const int32_t* x_v,
                                const double* x_len, const uint64_t* x_mask, const uint64_t* start_mask, const uint64_t* goal_mask,
                                uint64_t* reach, int32_t* goal_slice, int32_t* path_len, int32_t* path_node, int32_t* path_slice,
                                int32_t* sweeps);

/* ---- batched tree planner: bidirectional RRT-Connect for W worlds in one launch (tree_plan.hip) ---- */
/* The reference's single-query high-level planners (RRT_HLP, RRT_connect_HLP, robot_arm_RRT_HLP with HLP_grow_tree_mode = 'new'): a fresh
 * pair of trees per query, grown where the query is, with no graph built beforehand.  Everything geometric is the roadmap's, reused as it
 * stands: the node rule, the edge rule's sub-segments (S, midpoints, enlargements) and the wrapped distance.  Deterministic: a world's
 * result depends on its own inputs and seed alone, and the device and the host entry run the same functions.
 *
 * Trees.  Tree 0 is rooted at start, tree 1 at goal.  Nodes are kept UNWRAPPED: a continuous joint may leave [-pi, pi]; every difference
 *   of two configurations is the edge rule's D (wrapped on continuous joints), so that is harmless.
 * Random numbers.  Counter-based, arithmetic mod 2^64:
 *     u(seed, i, j):  z = seed + 0x9E3779B97F4A7C15 * (((i << 8) | j) + 1)
 *                     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31
 *                     u = (z >> 11) * 2^-53
 *   The sample of iteration i is qr_j = lb_j + u(seed, i, j) (ub_j - lb_j).
 * prefix(a, b) -> (m, S).  The edge rule's S sub-segments of the edge a -> b; m = the index of the first sub-segment whose enlarged test
 *   does not separate, m = S when all do.  Sub-segments 0 .. m - 1 cover q(t), t in [0, m / S], each by its own test, so the edge rule's
 *   soundness argument holds for that prefix unchanged: no configuration on a -> a + (m / S) D collides.
 * nearest(tree, q).  The node with the smallest (acc, index), acc = the squared wrapped distance node -> q (the sum of the nearest-
 *   neighbour search, without its square root): a total order, the smaller index on a tie.
 * The run of one world (cap = max_nodes):
 *     node rule at start, then at goal: not free -> START_BLOCKED / GOAL_BLOCKED, 0 iterations, no trees (count 0, 0)
 *     (m, S) = prefix(start, goal);  m == S -> FOUND, the path [start, goal], 0 iterations, no trees (as armour_roadmap_plan's direct edge)
 *     trees = {start}, {goal}
 *     for i = 0 .. max_iterations - 1:     a = i & 1 (the tree that extends), b = 1 - a
 *         either tree holds cap nodes -> TREE_FULL, iterations = i
 *         qr = the sample of i;  v = nearest(tree a, qr);  acc == 0 -> next i
 *         dist = sqrt(acc);  D = node v -> qr;  qn = node v + D when dist <= step, else node v + (step / dist) D
 *         (m, S) = prefix(node v, qn);  m == 0 -> next i;  m < S -> qn = node v + (m / S) D(node v -> qn)      (extend keeps the free prefix)
 *         append qn to tree a with parent v
 *         vb = nearest(tree b, qn);  (m, S) = prefix(node vb, qn)
 *         m == S -> FOUND, iterations = i + 1 (qn is NOT added to tree b);  m >= 1 -> append node vb + (m / S) D(node vb -> qn), parent vb
 *     NOT_FOUND, iterations = max_iterations
 *   m / S is fl(m) / fl(S) in fp64; fp64 throughout, no fused multiply-add.
 * Path.  start = tree 0's root, ..., the joining edge, ..., tree 1's root = goal, whichever tree extended last; consecutive equal points
 *   are possible.  Soundness: every segment of a returned path is a union of sub-segments whose enlarged tests separated (a tree edge is
 *   a free prefix, the joining edge a whole free edge), so no configuration on the path collides.
 * Limits (ARMOUR_EINVAL before a device is touched): W and O as armour_roadmap_check; 2 <= max_nodes <= ARMOUR_TREE_MAX_NODES;
 *   0 <= max_iterations <= ARMOUR_TREE_MAX_ITERATIONS; step, edge_step > 0 and finite; lb <= ub, finite; finite starts, goals and
 *   obstacles; max_points >= 0.  W = 0 is a success that does nothing.  ARMOUR_ECAPACITY when an edge of a run could have more than
 *   ARMOUR_TREE_MAX_SEGMENTS sub-segments: ceil(span_j / edge_step) with span_j = pi on a continuous joint and otherwise the extent of
 *   [lb_j, ub_j] and every start and goal (a new node lies between an old one and a sample).
 * Arrays are host pointers.  continuous [n] (NULL: robot->continuous); lb / ub [n] the sampling box; obstacles [W][O][12]; starts / goals
 *   [W][n]; seeds [W].  Outputs: status / iterations / points [W]; optional (NULL: not returned) path [W][max_points][n], count [W][2],
 *   nodes [W][2][max_nodes][n], parent [W][2][max_nodes] (-1 at a root), ms (device time of the launch).  Only the first count rows of a
 *   tree and the first points rows of a path are written.  When a found path has more than max_points points the call returns
 *   ARMOUR_ECAPACITY with points [W] complete and that world's path unwritten (the roadmap entries' rule; without path nothing is refused).
 * Device: one launch, grid W, a 256-lane block per world with the world's obstacles staged in LDS; the loop above runs inside the block,
 *   ordered by __syncthreads() alone -- no atomics, no flags, no block waits on another -- and is bounded by max_iterations.  The nearest
 *   scan deals the nodes to lanes and reduces (acc, index) by shuffles and LDS; a prefix takes its sub-segments in ascending chunks and
 *   stops at the first chunk with a hit; a short edge gives each sub-segment several lanes, each with a slice of the obstacles (the
 *   verdict of a sub-segment is the AND over obstacles, so nothing changes but the time).  W = 1 runs on one compute unit, and a launch
 *   lasts as long as its slowest world.  DESIGN.md 4.12c.
 * armour_tree_plan_host is the same functions in a loop and touches no device.  margin [W] (may be NULL): the smallest |clearance| over
 *   the checks that decided the world's run -- the two node checks and sub-segments 0 .. min(m, S - 1) of every prefix -- i.e. how far
 *   the run was from a verdict that rounding in sin / cos could flip (+inf when nothing was checked). */
#define ARMOUR_TREE_NOT_FOUND 0
#define ARMOUR_TREE_FOUND 1
#define ARMOUR_TREE_START_BLOCKED 2
#define ARMOUR_TREE_GOAL_BLOCKED 3
#define ARMOUR_TREE_FULL 4
#define ARMOUR_TREE_MAX_NODES 8192
#define ARMOUR_TREE_MAX_ITERATIONS 100000
#define ARMOUR_TREE_MAX_SEGMENTS 1048576
int armour_tree_plan(const ArmourRobot* robot, const uint8_t* continuous, const double* lb, const double* ub, int32_t W, int32_t O,
                     const double* obstacles, const double* starts, const double* goals, const uint64_t* seeds, double step, double edge_step,
                     int32_t max_iterations, int32_t max_nodes, int32_t max_points, int32_t* status, int32_t* iterations, int32_t* points,
                     double* path, int32_t* count, double* nodes, int32_t* parent, double* ms);
int armour_tree_plan_host(const ArmourRobot* robot, const uint8_t* continuous, const double* lb, const double* ub, int32_t W, int32_t O,
                          const double* obstacles, const double* starts, const double* goals, const uint64_t* seeds, double step, double edge_step,
                          int32_t max_iterations, int32_t max_nodes, int32_t max_points, int32_t* status, int32_t* iterations, int32_t* points,
                          double* path, int32_t* count, double* nodes, int32_t* parent, double* margin);
/* armour_tree_plan against obstacles in LINEAR MOTION, over a time window per world: the static entry with velocity [W][O][3], t_from and
 * t_to [W] after obstacles, which are the poses at world time 0 (armour_roadmap_check_moving's arguments).
 * The rule is armour_roadmap_check_moving's window rule and nothing else changes.  The host computes once per world mid[w] = 0.5 * (t_from[w]
 *   + t_to[w]) and half[w] = 0.5 * (t_to[w] - t_from[w]) and hands these two doubles to the kernel.  The node rule at start and goal and every
 *   sub-segment test of every prefix are the static ones with, for obstacle o, the box centre x - v_o mid[w] and every half-size
 *   h_l + (r_l + |v_o|_2 half[w]) (r_l = 0 for a node).  S, the sub-segment midpoints and enlargements, prefix, nearest, the steer step, the
 *   counter hash, the order of the loop and the path are word for word the static entry's.
 * Soundness.  Within [t_from, t_to] obstacle o leaves its pose of time mid by at most |v_o| half, so the static argument holds with the
 *   window in place of the instant: no configuration on a returned path meets an obstacle at ANY time of the window, whatever the time at
 *   which the arm passes it.  The trees do not carry time; a path is not a schedule.
 * With zero velocities every output is armour_tree_plan's bit for bit, for any window; t_from == t_to judges at an instant.
 * ARMOUR_EINVAL before a device is touched: armour_tree_plan's refusals; a null or non-finite velocity, t_from or t_to; t_from[w] > t_to[w].
 *   O = 0 with null obstacles and velocity is served as the static entry serves it.
 * Device: the static launch with RM_OBS_STRIDE + 4 doubles of LDS per obstacle (248 B: 62 KB per block at the cap, which the entry asks the
 *   runtime for); ARMOUR_ECAPACITY, without a launch, when the device grants a block less dynamic LDS than that beside the kernel's static.
 * armour_tree_plan_moving_host is the same functions in a loop and touches no device; margin [W] as armour_tree_plan_host's, of the
 *   window rule's clearances. */
int armour_tree_plan_moving(const ArmourRobot* robot, const uint8_t* continuous, const double* lb, const double* ub, int32_t W, int32_t O,
                            const double* obstacles, const double* velocity, const double* t_from, const double* t_to, const double* starts,
                            const double* goals, const uint64_t* seeds, double step, double edge_step, int32_t max_iterations, int32_t max_nodes,
                            int32_t max_points, int32_t* status, int32_t* iterations, int32_t* points, double* path, int32_t* count,
                            double* nodes, int32_t* parent, double* ms);
int armour_tree_plan_moving_host(const ArmourRobot* robot, const uint8_t* continuous, const double* lb, const double* ub, int32_t W, int32_t O,
                                 const double* obstacles, const double* velocity, const double* t_from, const double* t_to, const double* starts,
                                 const double* goals, const uint64_t* seeds, double step, double edge_step, int32_t max_iterations,
                                 int32_t max_nodes, int32_t max_points, int32_t* status, int32_t* iterations, int32_t* points, double* path,
                                 int32_t* count, double* nodes, int32_t* parent, double* margin);

/* ---- path shortening: W polylines in W worlds validated, pruned and refined in one launch (path_shortcut.hip) ---- */
/* What a user of a sampling planner expects back, and what the reference's HLPs need to reuse their last path (HLP_grow_tree_mode =
 * 'seed'): given a polyline per world, prove that every segment is still free and return a shorter polyline made of free segments.  It
 * applies to any path: the tree planner's, the roadmap's, a caller's own.  The tree planner's definitions are reused as they stand:
 * prefix(a, b) -> (m, S), the wrapped difference D(a -> b) and the wrapped distance.  An edge a -> b is FREE when m == S.  Points are kept
 * unwrapped and are never recomputed, except for inserted midpoints.  Deterministic; the device and the host entry run the same functions.
 *
 * One world, its path p_0 .. p_{P-1} (P >= 2), edge_step, passes >= 1:
 *   validate.  For s = 0 .. P - 2 in order the edge p_s -> p_{s+1} must be free.  The first s that is not gives status
 *     ARMOUR_SHORTCUT_INVALID, first_bad = s, points = 0, passes_done = 0, length_out = 0; the world's output rows are not written.
 *   prune(list).  i = 0, out = [p_0]; while i < last: j = the largest index > i whose edge p_i -> p_j is free, append p_j, i = j.
 *     j = i + 1 always qualifies and is taken untested: every edge of the list is known free when prune runs.  The verdict of a candidate
 *     is a pure function of its two end points, so the order of evaluation is the implementation's choice and does not show in the result.
 *   refine(list).  For every consecutive pair (a, b) whose points differ bitwise: mid_j = a_j + 0.5 D_j(a -> b) (fp64, no fused multiply-
 *     add), inserted only when a -> mid and mid -> b are both free by their own tests -- a whole edge's freedom is not inherited by its
 *     halves, each half has its own S and its own enlargements.  If 2 count - 1 > max_points, this refine and every later pass are skipped.
 *   the run.  validate; prune; then for each further pass: refine, prune.  Status ARMOUR_SHORTCUT_OK, first_bad = -1, passes_done = the
 *     number of prunes that ran.
 *   Soundness.  Every segment of an output path is an edge whose every sub-segment's enlarged test separated -- an input edge, a candidate
 *     that prune accepted or a half that refine accepted -- so no configuration on the output collides (the tree planner's argument).
 *   Length.  length_in / length_out = the sum of the wrapped distances of consecutive points, in index order, of the input and of the
 *     output.  Prune replaces a chain by the wrapped-shortest edge and refine splits an edge in two: length_out <= length_in up to rounding.
 * Limits (ARMOUR_EINVAL before a device is touched): W and O as armour_roadmap_check; 2 <= counts[w] <= max_in <=
 *   ARMOUR_SHORTCUT_MAX_POINTS; 2 <= max_points <= ARMOUR_SHORTCUT_MAX_POINTS; 1 <= passes <= ARMOUR_SHORTCUT_MAX_PASSES; edge_step > 0
 *   and finite; finite obstacles and points (the first counts[w] of a path; the padding is not read).  W = 0 is a success that does nothing.
 *   ARMOUR_ECAPACITY when an edge between any two points could have more than ARMOUR_TREE_MAX_SEGMENTS sub-segments: ceil(span_j /
 *   edge_step) with span_j = pi on a continuous joint and otherwise the extent of all the paths' points (a midpoint lies between two
 *   points); and when a world's pruned path has more than max_points points -- points [W] is then complete and that world's rows are
 *   unwritten (the roadmap entries' rule).
 * Arrays are host pointers.  paths [W][max_in][n], counts [W]; outputs status / points / first_bad / passes_done [W], length_in /
 *   length_out [W], out [W][max_points][n] (may be NULL; only the first points rows of a world are written), ms (may be NULL: device time
 *   of the launch).
 * Device: one launch, grid W, a 256-lane block per world, the world's obstacles and its path in LDS, ordered by __syncthreads() alone.
 *   validate, an anchor's prune candidates (j = last, last - 1, ...) and refine's halves are each a flat work list of (candidate,
 *   sub-segment) items laid across the lanes, several candidates to a chunk; prune stops at the first chunk after which some candidate is
 *   fully tested and free and every candidate above it has a hit.  DESIGN.md 4.12d.
 * armour_path_shortcut_host is the same functions in a loop and touches no device: validate in order, prune's candidates in descending j
 *   down to i + 2, refine's a -> mid and then (only when that is free) mid -> b, each with prefix.  margin [W] (may be NULL): the smallest
 *   |clearance| over the checks that evaluation made -- sub-segments 0 .. min(m, S - 1) of every prefix; +inf when nothing was checked. */
#define ARMOUR_SHORTCUT_OK 0
#define ARMOUR_SHORTCUT_INVALID 1
#define ARMOUR_SHORTCUT_MAX_POINTS 1024
#define ARMOUR_SHORTCUT_MAX_PASSES 8
int armour_path_shortcut(const ArmourRobot* robot, const uint8_t* continuous, int32_t W, int32_t O, const double* obstacles, int32_t max_in,
                         const double* paths, const int32_t* counts, double edge_step, int32_t passes, int32_t max_points, int32_t* status,
                         int32_t* points, int32_t* first_bad, int32_t* passes_done, double* out, double* length_in, double* length_out,
                         double* ms);
int armour_path_shortcut_host(const ArmourRobot* robot, const uint8_t* continuous, int32_t W, int32_t O, const double* obstacles,
                              int32_t max_in, const double* paths, const int32_t* counts, double edge_step, int32_t passes,
                              int32_t max_points, int32_t* status, int32_t* points, int32_t* first_bad, int32_t* passes_done, double* out,
                              double* length_in, double* length_out, double* margin);
/* armour_path_shortcut against obstacles in LINEAR MOTION, over a time window per world: the static entry with velocity [W][O][3], t_from
 * and t_to [W] after obstacles (the poses at world time 0).  An edge is FREE when every sub-segment passes the window rule's test, exactly
 * as armour_tree_plan_moving's prefix judges it (mid[w] and half[w] computed once on the host); validate, prune, refine, the midpoint, the
 * lengths and the order of the passes are word for word the static entry's.  Soundness: every segment of an output path is an edge whose
 * every sub-segment separated under the window rule, so no configuration on the output meets an obstacle at ANY time of [t_from, t_to],
 * whatever the time at which the arm passes it.  A path that was free in an earlier window can be INVALID in a later one: that is how a
 * planner that keeps its path learns that the world has moved over it.
 * With zero velocities every output column is armour_path_shortcut's bit for bit, for any window.
 * ARMOUR_EINVAL before a device is touched: armour_path_shortcut's refusals; a null or non-finite velocity, t_from or t_to;
 *   t_from[w] > t_to[w].  O = 0 with null obstacles and velocity is served as the static entry serves it.
 * Device: the static launch; dynamic LDS = O * 248 B of obstacles (62 KB at the cap) + max(max_in, max_points) * n * 8 B of path (up to
 *   64 KB) beside the kernel's static 21.6 KB, which the entry asks the runtime for; ARMOUR_ECAPACITY, without a launch, when the sum
 *   exceeds what the device grants a block.
 * armour_path_shortcut_moving_host is the same functions in a loop and touches no device; margin [W] as armour_path_shortcut_host's, of
 *   the window rule's clearances. */
int armour_path_shortcut_moving(const ArmourRobot* robot, const uint8_t* continuous, int32_t W, int32_t O, const double* obstacles,
                                const double* velocity, const double* t_from, const double* t_to, int32_t max_in, const double* paths,
                                const int32_t* counts, double edge_step, int32_t passes, int32_t max_points, int32_t* status, int32_t* points,
                                int32_t* first_bad, int32_t* passes_done, double* out, double* length_in, double* length_out, double* ms);
int armour_path_shortcut_moving_host(const ArmourRobot* robot, const uint8_t* continuous, int32_t W, int32_t O, const double* obstacles,
                                     const double* velocity, const double* t_from, const double* t_to, int32_t max_in, const double* paths,
                                     const int32_t* counts, double edge_step, int32_t passes, int32_t max_points, int32_t* status,
                                     int32_t* points, int32_t* first_bad, int32_t* passes_done, double* out, double* length_in,
                                     double* length_out, double* margin);

/* ---- batched collision-aware inverse kinematics for workspace goals (ik.hip) ---- */
/* The reference's end-effector planner (arm_end_effector_RRT_star_HLP) takes its goal and waypoints as points of the workspace and turns
 * each into a configuration with agent_info.inverse_kinematics(z, q_0): position only, inside the joint limits, started from a guess.  The
 * arm is redundant (3 equations, up to ARMOUR_MAX_FACTORS joints), so which solution is useful depends on the world (it must be free) and
 * on where the arm is (it should be near): N targets are solved from S start points each, every converged solution is judged by the node
 * rule against its target's world, and one is picked per target.  Frames, the node rule and the wrapped distance are the roadmap's, the
 * counter hash u(seed, i, j) is the tree planner's.  Deterministic; the device and the host entry run the same functions.
 *
 * One ITEM is (target t, seed s), s = 0 .. S - 1.  fp64 throughout, no fused multiply-add; dot(a, b) = (a0 b0 + a1 b1) + a2 b2.
 * End-effector point p(q).  R = I, p = 0; for l = 0 .. J - 1 the roadmap's step along the chain (link l's translation, rpy, joint
 *   rotation) gives the frame R_l, o_l of link l.  p(q) = o_{J-1} + R_{J-1} tool, row i: o_i + ((R_i0 tool_0 + R_i1 tool_1) + R_i2 tool_2).
 *   tool = 0 is the last frame's origin (the reference's J(:, end)).
 * Position Jacobian.  Column j of an actuated joint (j < n, axis_j != 0) is c_j = a_j x (p(q) - o_j), a_j = sign(axis_j) times the column
 *   |axis_j| - 1 of R_j (the joint's world axis), the difference taken component by component and the cross product as the node rule
 *   writes it (m0 = a1 d2 - a2 d1, ...).  A joint that is not actuated has no column (c_j = 0).
 * Start point.  s = 0: q_j = q_ref[t][j].  s >= 1: q_j = lb_j + u(seeds[t], s, j) (ub_j - lb_j).  Then every non-continuous joint is
 *   clipped, q_j = min(max(q_j, lb_j), ub_j); continuous joints are kept unwrapped, as tree nodes are.
 * Iteration, k = 0, 1, ...:
 *     e = target - p(q);  err = sqrt(dot(e, e))
 *     err <= tol            -> CONVERGED, iterations = k
 *     k == max_iterations   -> not converged, iterations = k
 *     err > e_max           -> sc = e_max / err;  e_i = e_i sc
 *     A = J J^T + lambda^2 I (3 x 3): A_ik = 0, then + c_j[i] c_j[k] for j = 0 .. n - 1 in order, then A_ii + lambda lambda
 *     Cholesky A = L L^T:  L00 = sqrt(A00); L10 = A10 / L00; L20 = A20 / L00; L11 = sqrt(A11 - L10 L10); L21 = (A21 - L20 L10) / L11;
 *                          L22 = sqrt((A22 - L20 L20) - L21 L21)
 *     L z = e:    z0 = e0 / L00; z1 = (e1 - L10 z0) / L11; z2 = ((e2 - L20 z0) - L21 z1) / L22
 *     L^T y = z:  y2 = z2 / L22; y1 = (z1 - L21 y2) / L11; y0 = ((z0 - L10 y1) - L20 y2) / L00
 *     q_j = q_j + dot(c_j, y), then the clip of the start point
 *   This is the damped least-squares step with a clamped error and a fixed lambda; no step is rejected.  The item's outputs are q, err and
 *   iterations as the iteration left them.
 * Free test.  A converged item is FREE when the node rule at q (no enlargement) separates every link box from every obstacle of world
 *   world[t]; world[t] = -1 means no obstacles.  flags: bit 0 converged, bit 1 free (0 when not converged).
 * Pick.  Among the items of target t with both bits, the one with the smallest (acc, s), acc = the squared wrapped distance q_ref[t] -> q
 *   (the tree planner's order: a total order).  best[t] = that s and q_best[t] = its q; best[t] = -1 and the row unwritten with none.
 *   status[t]: ARMOUR_IK_FOUND; ARMOUR_IK_ALL_BLOCKED (some item converged, none is free); ARMOUR_IK_NONE_CONVERGED.
 * Limits (ARMOUR_EINVAL before a device is touched): 0 <= N <= ARMOUR_IK_MAX_TARGETS; 1 <= S <= ARMOUR_IK_MAX_SEEDS;
 *   0 <= max_iterations <= ARMOUR_IK_MAX_ITERATIONS; lambda, e_max, tol > 0 and finite; lb <= ub, finite; finite targets, q_ref, tool and
 *   obstacles; W and O as armour_roadmap_check; -1 <= world[t] < W.  N = 0 is a success that does nothing.
 * Arrays are host pointers.  continuous [n] (NULL: robot->continuous); lb / ub [n]; tool [3]; obstacles [W][O][12]; world [N]; targets
 *   [N][3]; q_ref [N][n]; seeds [N].  Outputs: status / best [N], q_best [N][n]; optional (NULL: not returned) q [N][S][n], err [N][S],
 *   iterations [N][S], flags [N][S], ms (device time of the launch).
 * Device: one launch, grid N, a 256-lane block per target with the world's obstacles staged in LDS, ordered by __syncthreads() alone --
 *   no atomics, no block waits on another.  Lane s solves item s; up to 128 seeds the free test of an item is shared by G = min(O, 256 / S)
 *   lanes, lane g with the obstacles [g O / G, (g + 1) O / G) (the verdict is the AND over obstacles, so nothing changes but the time);
 *   the pick is a reduction of (acc, s) by shuffles and LDS.  N = 1 runs on one compute unit, and a launch lasts as long as its slowest
 *   item.  DESIGN.md 4.12e.
 * armour_ik_host is the same functions in a loop and touches no device.  margin [N] (may be NULL): the smallest |clearance| of the node
 *   rule over the target's converged items -- how far the free verdicts were from one that rounding in sin / cos could flip (+inf when no
 *   item converged or the world has no obstacles).
 * armour_ik_end_effector_host: p [N][3] = p(q[i]) and, unless NULL, jac [N][3][n] (row r, column j = c_j[r]) for q [N][n]; host only. */
#define ARMOUR_IK_NONE_CONVERGED 0
#define ARMOUR_IK_FOUND 1
#define ARMOUR_IK_ALL_BLOCKED 2
#define ARMOUR_IK_MAX_SEEDS 256
#define ARMOUR_IK_MAX_ITERATIONS 1000
#define ARMOUR_IK_MAX_TARGETS 1048576
int armour_ik(const ArmourRobot* robot, const uint8_t* continuous, const double* lb, const double* ub, const double* tool, int32_t N, int32_t S,
              int32_t W, int32_t O, const double* obstacles, const int32_t* world, const double* targets, const double* q_ref,
              const uint64_t* seeds, double lambda, double e_max, double tol, int32_t max_iterations, int32_t* status, int32_t* best,
              double* q_best, double* q, double* err, int32_t* iterations, int32_t* flags, double* ms);
int armour_ik_host(const ArmourRobot* robot, const uint8_t* continuous, const double* lb, const double* ub, const double* tool, int32_t N,
                   int32_t S, int32_t W, int32_t O, const double* obstacles, const int32_t* world, const double* targets, const double* q_ref,
                   const uint64_t* seeds, double lambda, double e_max, double tol, int32_t max_iterations, int32_t* status, int32_t* best,
                   double* q_best, double* q, double* err, int32_t* iterations, int32_t* flags, double* margin);
/* armour_ik against obstacles in LINEAR MOTION, over a time window per world: the static entry with velocity [W][O][3], t_from and t_to [W]
 * after obstacles, which are the poses at world time 0 (armour_roadmap_check_moving's arguments).
 * The rule.  The free test of a converged item of target t is the node rule over the window of the target's world w = world[t]:
 *   armour_roadmap_check_moving's window rule at (mid[w], half[w]) = (0.5 (t_from[w] + t_to[w]), 0.5 (t_to[w] - t_from[w])), computed once on
 *   the host -- for obstacle o the box centre x - v_o mid[w] and every half-size h_l + |v_o|_2 half[w].  world[t] = -1 has no obstacles and
 *   reads no window.  The start points, the damped least-squares iteration, convergence and the pick are word for word the static entry's.
 * Soundness.  Within [t_from, t_to] obstacle o leaves its pose of time mid by at most |v_o| half, so a configuration that is IK_FOUND meets no
 *   obstacle of its world at ANY time of the window.
 * With zero velocities every output is armour_ik's bit for bit, for any window; t_from == t_to judges at an instant.
 * ARMOUR_EINVAL before a device is touched: armour_ik's refusals; a null or non-finite velocity, t_from or t_to; t_from[w] > t_to[w].  N = 0
 *   and W = 0 are served as the static entry serves them.
 * Device: the static launch with RM_OBS_STRIDE + 4 doubles of LDS per obstacle (62 KB per block at the cap, which the entry asks the runtime
 *   for); ARMOUR_ECAPACITY, without a launch, when the device grants a block less.
 * armour_ik_moving_host is the same functions in a loop and touches no device; margin [N] as armour_ik_host's, of the window rule's clearances. */
int armour_ik_moving(const ArmourRobot* robot, const uint8_t* continuous, const double* lb, const double* ub, const double* tool, int32_t N,
                     int32_t S, int32_t W, int32_t O, const double* obstacles, const double* velocity, const double* t_from, const double* t_to,
                     const int32_t* world, const double* targets, const double* q_ref, const uint64_t* seeds, double lambda, double e_max,
                     double tol, int32_t max_iterations, int32_t* status, int32_t* best, double* q_best, double* q, double* err,
                     int32_t* iterations, int32_t* flags, double* ms);
int armour_ik_moving_host(const ArmourRobot* robot, const uint8_t* continuous, const double* lb, const double* ub, const double* tool, int32_t N,
                          int32_t S, int32_t W, int32_t O, const double* obstacles, const double* velocity, const double* t_from,
                          const double* t_to, const int32_t* world, const double* targets, const double* q_ref, const uint64_t* seeds,
                          double lambda, double e_max, double tol, int32_t max_iterations, int32_t* status, int32_t* best, double* q_best,
                          double* q, double* err, int32_t* iterations, int32_t* flags, double* margin);
int armour_ik_end_effector_host(const ArmourRobot* robot, int32_t N, const double* q, const double* tool, double* p, double* jac);

/* ---- batched workspace RRT*: the end-effector planner's tree for W worlds in one launch (ws_tree.hip) ---- */
/* The reference's experiments plan their waypoints with arm_end_effector_RRT_star_HLP: an RRT* grown in the 3-D workspace for the
 * end-effector POINT (RRT_HLP.m, RRT_star_HLP.m), whose best path is followed for a lookahead distance and turned into a configuration by
 * inverse kinematics (armour_ik).  This entry grows that tree, W worlds at a time.  Deterministic: a world's result depends on its own
 * inputs and seed alone, and the device and the host entry run the same functions.  fp64 throughout, no fused multiply-add;
 * dot(a, b) = (a0 b0 + a1 b1) + a2 b2 as the inverse kinematics writes it.
 *
 * Point rule.  A point x with buffer b >= 0 is the box with centre x, axes e_0, e_1, e_2 and half-sizes (b, b, b); it is tested against an
 *   obstacle by the roadmap's pair test as it stands (verdict mode), and x is FREE when every obstacle of the world separates.  The
 *   reference inflates its axis-aligned boxes by 2 b per side (arm_end_effector_RRT_star_HLP.m:117): the same set for those boxes, and
 *   this form is defined for the general obstacle [c g1 g2 g3] as well.  Nothing geometric is restated.
 * Edge rule (conservative, sound).  The edge a -> b:  D = b - a component by component, len = sqrt(dot(D, D)),
 *   S = min(ARMOUR_WS_MAX_SEGMENTS, max(1, ceil(len / edge_step))).  Sub-segment s = 0 .. S - 1 is tested as the box with centre a + t_s D,
 *   t_s = fl(2 s + 1) / fl(2 S), and half-sizes b + |D_i| / fl(2 S): the exact bounding box of the sub-segment, grown by the buffer, so a
 *   sub-segment whose test separates touches no buffered obstacle -- for any S >= 1, which is why the cap on S costs resolution and not
 *   soundness.  prefix(a, b) -> (m, S) as in the tree planner (m = the first sub-segment that does not separate, S when all do); the edge
 *   is FREE when m == S.  An edge is always tested in the direction existing node -> new point: one test serves the parent choice and
 *   the rewire.
 * Samples.  u(seed, i, j) is the tree planner's.  In iteration i: u(seed, i, 3) < goal_rate -> the sample is the goal; otherwise
 *   qr_j = lb_j + u(seed, i, j) (ub_j - lb_j), j = 0 .. 2.
 * The run of one world (cap = max_nodes; a node holds x, parent, len = the length of its parent edge, and cost):
 *     point rule at start: not free -> START_BLOCKED, 0 iterations, count 0, no path (path_cost 0, goal_dist = |goal - start|)
 *     tree = {start}: cost 0, len 0, parent -1
 *     initial chain (init, init_count[w] >= 1; the reference's 'seed' mode, RRT_HLP.m:104-107): chain point c = 0, 1, ... is appended with
 *       parent = the node appended before it (the root for c = 0), len = d, cost = cost_parent + d, d = the edge's len, while that edge is
 *       free and the tree is not full; the first edge that is not free ends the chain.  chain_kept = how many were appended.
 *     for i = 0 .. max_iterations - 1:
 *         the tree holds cap nodes -> stop, iterations = i
 *         qr = the sample of i;  v = the node with the smallest (acc, index), acc = dot(D, D), D = qr - x_v;  acc == 0 -> next i
 *         dist = sqrt(acc);  qn = qr when dist <= step, else qn_j = x_v_j + (step / dist) D_j
 *         candidates = every node c with acc_c <= rewire_radius rewire_radius (acc_c: from x_c to qn), and v.  rewire_radius = 0: plain RRT.
 *         for each candidate c:  d_c = sqrt(acc_c);  c is free when the edge x_c -> qn is FREE
 *         no candidate is free -> next i
 *         parent p = the free candidate with the smallest (cost_c + d_c, c);  append qn with len = d_p, cost = cost_p + d_p
 *         rewire: every other free candidate c with cost_qn + d_c < cost_c (the costs as they were before any rewire of this iteration)
 *           gets parent = qn, len = d_c;  rewires counts them
 *         after any rewire the costs are re-derived so that cost_k = fl(cost_parent(k) + len_k) holds for every node, bit for bit: a
 *           recursive definition from the root, independent of the schedule that reaches it
 *     iterations = max_iterations when the loop ends by itself
 *   Best node.  g_k = sqrt(acc), acc from x_k to goal.  Among the nodes with g_k <= goal_tol the smallest (cost_k + g_k, k): status REACHED.
 *     With none, the smallest (acc, k): status PARTIAL, the reference's "path to the node closest to the goal" (RRT_HLP.m:267-299).
 *     The path runs root -> best node (points of them); path_cost = the best node's cost, goal_dist = its g.
 * Two deliberate departures from RRT_star_HLP.m:
 *   Parent choice.  The reference picks the candidate parent by min(cost) alone (:110); here it is cost + distance, RRT* as published.
 *   Stale costs.  After a rewire the reference never updates the rewired node's cost nor its descendants' (:147-153), which is how its
 *     tree can come to hold a loop ("The RRT has a loop in it by accident!", RRT_HLP.m:308).  With re-derived costs no cycle can form:
 *     costs are monotone along a branch, because fl(a + d) >= a for d >= 0; so an ancestor c of qn has cost_c <= cost_qn and cannot pass
 *     the strict test cost_qn + d_c < cost_c; so every rewired node gets a parent (qn, a new leaf) that is not its descendant, and qn's
 *     own chain to the root holds no rewired node.  The structure stays a tree rooted at start.
 *   Soundness of the path: every tree edge -- a chain edge, a parent edge, a rewired edge -- is an edge whose every sub-segment's test
 *     separated, so no point of a returned path, grown by the buffer, touches an obstacle.
 * Limits (ARMOUR_EINVAL before a device is touched): W and O as armour_roadmap_check; 1 <= max_nodes <= ARMOUR_WS_MAX_NODES;
 *   0 <= max_iterations <= ARMOUR_TREE_MAX_ITERATIONS; step, edge_step > 0; rewire_radius, buffer, goal_tol >= 0; 0 <= goal_rate <= 1; all
 *   finite; lb <= ub, finite; finite starts, goals, chains and obstacles; 0 <= init_count[w] <= max_init (>= 1) when init is given;
 *   ceil(max(step, rewire_radius) / edge_step) and ceil(len / edge_step) of every chain edge at most ARMOUR_WS_MAX_SEGMENTS (1024: a
 *   1 m edge at 1 mm), so that no bound of a work list depends on what the run does; max_points >= 0.  When a path has more than max_points
 *   points the call returns ARMOUR_ECAPACITY with points [W] complete and that world's rows unwritten (the roadmap entries' rule; without
 *   path nothing is refused).  W = 0 is a success that does nothing.
 * Arrays are host pointers.  lb / ub [3] the sampling box; obstacles [W][O][12]; starts / goals [W][3]; seeds [W]; optional init
 *   [W][max_init][3] with init_count [W] (init NULL: no chains).  Outputs: status / iterations / points / rewires / chain_kept [W],
 *   path_cost / goal_dist [W]; optional (NULL: not returned) path [W][max_points][3], count [W], nodes [W][max_nodes][3], parent
 *   [W][max_nodes] (-1 at the root), node_cost [W][max_nodes], ms (device time of the launch).  Only the first count rows of a tree and
 *   the first points rows of a path are written.
 * Device: one launch, grid W, a 256-lane block per world with the world's obstacles staged in LDS; the loop above runs inside the block,
 *   ordered by __syncthreads() alone -- no atomics, no flags, no block waits on another.  The tree lives in global memory, written and
 *   read by its block alone.  The nearest scan and the near set deal the nodes to lanes; the candidates' sub-segments are one flat work
 *   list across the lanes, 256 candidates to a round, and a short list gives each item several lanes, each with a slice of the obstacles
 *   (the verdict of a sub-segment is the AND over obstacles, so nothing changes but the time); the parent is a reduction, every free
 *   candidate decides its own rewire, and the costs are re-derived in passes that read the pass before until one changes nothing.
 *   RRT* runs a fixed number of iterations, so the blocks of a launch do comparable work; W = 1 runs on one compute unit.
 *   DESIGN.md 4.12f.
 * armour_ws_tree_plan_host is the same functions in a loop and touches no device.  margin [W] (may be NULL): the smallest |clearance|
 *   (per box: the minimum over the world's obstacles of the pair clearance) over the checks that decided -- the start point and
 *   sub-segments 0 .. min(m, S - 1) of every prefix; +inf when nothing was checked or the world has no obstacles. */
#define ARMOUR_WS_PARTIAL 0
#define ARMOUR_WS_REACHED 1
#define ARMOUR_WS_START_BLOCKED 2
#define ARMOUR_WS_MAX_NODES 4096
#define ARMOUR_WS_MAX_SEGMENTS 1024
int armour_ws_tree_plan(const double* lb, const double* ub, int32_t W, int32_t O, const double* obstacles, const double* starts,
                        const double* goals, const uint64_t* seeds, int32_t max_init, const double* init, const int32_t* init_count,
                        double step, double edge_step, double rewire_radius, double goal_rate, double buffer, double goal_tol,
                        int32_t max_iterations, int32_t max_nodes, int32_t max_points, int32_t* status, int32_t* iterations, int32_t* points,
                        int32_t* rewires, int32_t* chain_kept, double* path_cost, double* goal_dist, double* path, int32_t* count,
                        double* nodes, int32_t* parent, double* node_cost, double* ms);
int armour_ws_tree_plan_host(const double* lb, const double* ub, int32_t W, int32_t O, const double* obstacles, const double* starts,
                             const double* goals, const uint64_t* seeds, int32_t max_init, const double* init, const int32_t* init_count,
                             double step, double edge_step, double rewire_radius, double goal_rate, double buffer, double goal_tol,
                             int32_t max_iterations, int32_t max_nodes, int32_t max_points, int32_t* status, int32_t* iterations,
                             int32_t* points, int32_t* rewires, int32_t* chain_kept, double* path_cost, double* goal_dist, double* path,
                             int32_t* count, double* nodes, int32_t* parent, double* node_cost, double* margin);
/* armour_ws_tree_plan against obstacles in LINEAR MOTION, over a time window per world: the static entry with velocity [W][O][3], t_from and
 * t_to [W] after obstacles, which are the poses at world time 0 (armour_roadmap_check_moving's arguments).
 * The rule.  The host computes once per world mid[w] = 0.5 * (t_from[w] + t_to[w]) and half[w] = 0.5 * (t_to[w] - t_from[w]).  Every box the
 *   static rule tests -- the point rule's box at the start, every sub-segment box of the edge rule (centre x, axes e_0 e_1 e_2, half-sizes h)
 *   -- is tested against obstacle o as the box of centre x - v_o mid[w] and half-sizes h_i + |v_o|_2 half[w], each product and sum rounded on
 *   its own.  The samples, nearest, the steer step, the near set, the parent choice, rewiring, the cost re-derivation, the best node, the path
 *   and the initial chain (which ends at its first edge that the window blocks) are word for word the static entry's.
 * Soundness.  Within [t_from, t_to] obstacle o leaves its pose of time mid by at most |v_o| half in the 2-norm, and growing the box by that
 *   amount along every axis covers it: no point of a returned path, grown by the buffer, meets an obstacle at ANY time of the window,
 *   whatever the time at which the end effector passes it.  The trees do not carry time; a path is not a schedule.
 * With zero velocities every output is armour_ws_tree_plan's bit for bit, for any window; t_from == t_to judges at an instant.
 * ARMOUR_EINVAL before a device is touched: armour_ws_tree_plan's refusals; a null or non-finite velocity, t_from or t_to;
 *   t_from[w] > t_to[w].  W = 0 is served as the static entry serves it.
 * Device: the static launch with RM_OBS_STRIDE + 4 doubles of LDS per obstacle (62 KB per block at the cap, which the entry asks the runtime
 *   for); ARMOUR_ECAPACITY, without a launch, when the device grants a block less.
 * armour_ws_tree_plan_moving_host is the same functions in a loop and touches no device; margin [W] as armour_ws_tree_plan_host's, of the
 *   window rule's clearances.
 * The resident trees below (armour_ws_trees_*) stay static: a kept tree's edges were proved against the world as it stood, and a window that
 *   has passed proves nothing about the next. */
int armour_ws_tree_plan_moving(const double* lb, const double* ub, int32_t W, int32_t O, const double* obstacles, const double* velocity,
                               const double* t_from, const double* t_to, const double* starts, const double* goals, const uint64_t* seeds,
                               int32_t max_init, const double* init, const int32_t* init_count, double step, double edge_step,
                               double rewire_radius, double goal_rate, double buffer, double goal_tol, int32_t max_iterations, int32_t max_nodes,
                               int32_t max_points, int32_t* status, int32_t* iterations, int32_t* points, int32_t* rewires, int32_t* chain_kept,
                               double* path_cost, double* goal_dist, double* path, int32_t* count, double* nodes, int32_t* parent,
                               double* node_cost, double* ms);
int armour_ws_tree_plan_moving_host(const double* lb, const double* ub, int32_t W, int32_t O, const double* obstacles, const double* velocity,
                                    const double* t_from, const double* t_to, const double* starts, const double* goals, const uint64_t* seeds,
                                    int32_t max_init, const double* init, const int32_t* init_count, double step, double edge_step,
                                    double rewire_radius, double goal_rate, double buffer, double goal_tol, int32_t max_iterations,
                                    int32_t max_nodes, int32_t max_points, int32_t* status, int32_t* iterations, int32_t* points, int32_t* rewires,
                                    int32_t* chain_kept, double* path_cost, double* goal_dist, double* path, int32_t* count, double* nodes,
                                    int32_t* parent, double* node_cost, double* margin);

/* ---- resident workspace trees: the same trees kept between calls and grown in instalments (ws_tree.hip) ---- */
/* The reference's grow_tree_mode = 'keep' (RRT_HLP.m:99-117; the mode of kinova_run_hard_scenarios.m): the tree planted at the first call
 * stays and every later call grows it further, so the path is an anytime RRT* path.  An ArmourWsTrees holds the trees of W worlds whose
 * obstacles, goals, seeds and parameters are fixed at create; a grow runs further iterations of armour_ws_tree_plan's loop on the worlds it
 * lists; a read returns stored trees.
 * The defining property.  For any world, let its grows have had the iteration counts n_1, n_2, ..., n_k, the first of them having planted
 *   it from the point s.  Then the stored tree (read), the cumulative iterations and rewires, and the last grow's status, points, path,
 *   path_cost and goal_dist equal BIT FOR BIT what armour_ws_tree_plan / _host return for starts = s, no chain and max_iterations = sum n,
 *   on a host handle and on the device: a world's whole state between iterations is its node arrays, its count, its iteration index and
 *   its rewires, and the sample of iteration i is a function of (seed, i) alone.
 * armour_ws_trees_create / _create_host: lb, ub, W, O, obstacles [W][O][12], goals [W][3], seeds [W] and the parameters are
 *   armour_ws_tree_plan's and are refused by the same rules (ARMOUR_EINVAL; one copy of that code).  Every tree starts empty: count 0, 0
 *   iterations done.  Neither touches a device: a device handle uploads its worlds and reserves W max_nodes nodes with the first grow that
 *   launches.  _create_host makes the host form, whose grows run armour_ws_tree_plan_host's loop.
 * armour_ws_trees_grow: slot l = 0 .. L - 1 serves world worlds[l]; every output is [L], in slot order.
 *     the world's tree is empty: the point rule at starts[l]; not free -> START_BLOCKED, the tree stays empty, no iteration is consumed
 *       (goal_dist = |goal - starts[l]|), and a later call may plant it from another point; free -> starts[l] is the root.
 *     the world's tree is planted: starts[l] is not read.
 *     then `iterations` further iterations of the loop, i continuing from the world's iterations done; the world stops when its tree holds
 *       max_nodes nodes.  Then the best node and the path, as in armour_ws_tree_plan.
 *   iterations [L] and rewires [L] returned are cumulative; count [L] (may be NULL) the tree's nodes.  iterations = 0 is allowed: it plants
 *   the root, or returns the current path.  path [L][max_points][3] (may be NULL) and ARMOUR_ECAPACITY: armour_ws_tree_plan's rule, by slot.
 *   ms (may be NULL): the device time of the launch, 0 on a host handle.  margin [L] (may be NULL): a host handle's, the smallest
 *   |clearance| over THIS call's deciding checks.
 *   ARMOUR_EINVAL before a device is touched: an index outside [0, W); a world listed twice (two blocks would write one tree);
 *   iterations outside [0, ARMOUR_TREE_MAX_ITERATIONS]; max_points < 0; a world's iterations done + iterations beyond INT32_MAX; a start of
 *   an empty tree that is absent or not finite; margin on a device handle.  L = 0 is a success that does nothing.
 *   Device: ONE launch of grid L of the kernel of armour_ws_tree_plan in its resumed form -- block l takes w from the index list, loads
 *   the world's count, iteration base and rewires, skips the start test when the tree is planted, and writes the three words back at the
 *   end; nothing else differs, and the loop's first barrier orders the writes of the launch before as it orders an iteration's.  Nothing
 *   but the index list and the starts is uploaded.
 * armour_ws_trees_read: nodes [L][max_nodes][3], parent [L][max_nodes], node_cost [L][max_nodes], count [L] of the listed worlds (each may
 *   be NULL; a world may be listed twice); only the first count rows of a slot are written.
 * A handle is used by one thread at a time.  Out of scope: obstacles that change, re-rooting or pruning, a reset.  DESIGN.md 4.12g. */
typedef struct ArmourWsTrees ArmourWsTrees;
int armour_ws_trees_create(const double* lb, const double* ub, int32_t W, int32_t O, const double* obstacles, const double* goals,
                           const uint64_t* seeds, double step, double edge_step, double rewire_radius, double goal_rate, double buffer,
                           double goal_tol, int32_t max_nodes, ArmourWsTrees** out);
int armour_ws_trees_create_host(const double* lb, const double* ub, int32_t W, int32_t O, const double* obstacles, const double* goals,
                                const uint64_t* seeds, double step, double edge_step, double rewire_radius, double goal_rate, double buffer,
                                double goal_tol, int32_t max_nodes, ArmourWsTrees** out);
void armour_ws_trees_destroy(ArmourWsTrees* trees);
int armour_ws_trees_grow(ArmourWsTrees* trees, int32_t L, const int32_t* worlds, const double* starts, int32_t iterations, int32_t max_points,
                         int32_t* status, int32_t* iterations_done, int32_t* points, int32_t* rewires, double* path_cost, double* goal_dist,
                         double* path, int32_t* count, double* ms, double* margin);
int armour_ws_trees_read(ArmourWsTrees* trees, int32_t L, const int32_t* worlds, double* nodes, int32_t* parent, double* node_cost,
                         int32_t* count);
/* Test hook: sets the iterations that world `world` counts as done (>= 0), so that a test reaches the INT32_MAX rule of a grow without
 * running 2^31 iterations.  ARMOUR_ESTATE once a device handle has launched (its state is on the device then). */
int armour_debug_ws_trees_set_iterations(ArmourWsTrees* trees, int32_t world, int32_t done);

/* ---- path audit: executed pieces of Bezier plans checked against worlds' obstacles on the device (path_audit.hip) ---- */
/* The world's half of the safety claim (KSI/kinova_world_static.m collision_check after every move of KSI/simulator_armtd.m): did the path
 * the arm was sent along touch an obstacle?  P pieces are audited in one launch.  Piece p is the plan of armour_desired_trajectory
 * (q0[p], qd0[p], qdd0[p], end q0 + k_range .* k[p], `duration`) on the time window [ta[p], tb[p]] within [0, duration], in world
 * world_of_piece[p] of obstacles [W][O][12], with an optional tube radius e = tube[p] per joint (NULL: zeros) -- how far the executed
 * joint angles may be from the plan, e.g. the controller's ultimate bound.  Geometry, the node rule and rho_{j,l} are the roadmap's (above).
 *
 * Sub-intervals.  The plan's joint j is a degree-5 Bezier curve in s = t / duration with control points P_0..P_5 (P_0 = q0,
 * P_1 = q0 + a/5, P_2 = q0 + 2a/5 + b/20, P_3 = P_4 = P_5 = q0 + k_range k; a = qd0 duration, b = qdd0 duration^2).  Its derivative is the
 * degree-4 curve with control points 5 (P_{i+1} - P_i), so by the convex-hull property
 *   v_j = max_i |5 (P_{i+1,j} - P_{i,j})| / duration  >=  |qd_j(t)|  for every t in [0, duration].
 * The window is cut into S = max(1, ceil(max_j v_j (tb - ta) / step)) sub-intervals; sub-interval s has the midpoint
 * t_s = ta + (2s + 1)(tb - ta) / (2S).
 * Sample test (exact).  The node rule at q(t_s) with the link boxes as they are.  clearance <= 0 there is a PROVED collision of the
 * nominal path at t_s.
 * Tube test (conservative).  The node rule at q(t_s) with every half-size of link l enlarged by
 *   r_l = sum over actuated j <= l of rho_{j,l} (v_j (tb - ta) / (2S) + e_j).
 * Soundness, as for the edge rule: on sub-interval s the plan's joint j is within v_j (tb - ta)/(2S) of q_j(t_s) (mean value theorem with
 * the bound v_j), so every configuration within e of the plan there has joint j within v_j (tb - ta)/(2S) + e_j of q_j(t_s); turning the
 * joints there one at a time moves every point of link l by at most rho_{j,l} times the angle, so link l stays inside the box with
 * half-sizes h_l + r_l about the midpoint box.  If every enlarged box of every sub-interval is separated from every obstacle, no
 * configuration within e of the plan collides anywhere on the window.  (Rounding only helps: a plane's numerator is monotone in the
 * half-sizes in floating point too, so an item whose tube test separates has a separated sample test.)
 * Verdict per piece:  0 PROVED FREE (every tube test separates);  1 PROVED HIT (some sample test collides; t_hit = the first such t_s);
 *   2 UNDECIDED (neither).  Verdict 2 is NOT a finding: it says the audit at this `step` could not prove the piece free -- the tube came
 *   within r_l of an obstacle -- and nothing about a collision.  A smaller step shrinks r_l towards rho e and leaves fewer pieces
 *   undecided, for proportionally more work items; with e > 0, a piece closer than rho e to an obstacle stays undecided at every step.
 * Device.  One launch; a work item is one (piece, sub-interval) with its own Bezier evaluation and forward-kinematics pass, pieces are
 * grouped by world and a block serves one world (obstacles staged in LDS once); fp64 throughout.  A piece's result does not depend on the
 * other pieces of the call.  Arrays are host pointers: world_of_piece / ta / tb [P], q0 / qd0 / qdd0 / k / tube [P][n], k_range [n],
 * obstacles [W][O][12] with O <= ARMOUR_ROADMAP_MAX_OBSTACLES.  Outputs: verdict [P]; t_hit [P] (NaN unless verdict 1; may be NULL);
 * clearance [P] = the minimum sample-test clearance of the piece (may be NULL; when requested no item exits early); ms = device time of
 * the launch (may be NULL).  ARMOUR_EINVAL on a bad argument (checked before the device is touched), ARMOUR_ECAPACITY when the pieces have
 * more than 2^31 - 2 sub-intervals in all. */
int armour_path_audit(const ArmourRobot* robot, int32_t W, int32_t O, const double* obstacles, int32_t P, const int32_t* world_of_piece,
                      const double* q0, const double* qd0, const double* qdd0, const double* k, const double* k_range, double duration,
                      const double* ta, const double* tb, const double* tube, double step, int32_t* verdict, double* t_hit, double* clearance,
                      double* ms);
/* the same rule by the same functions in a host loop (for tests; runs without a GPU) */
int armour_path_audit_host(const ArmourRobot* robot, int32_t W, int32_t O, const double* obstacles, int32_t P, const int32_t* world_of_piece,
                           const double* q0, const double* qd0, const double* qdd0, const double* k, const double* k_range, double duration,
                           const double* ta, const double* tb, const double* tube, double step, int32_t* verdict, double* t_hit,
                           double* clearance);
/* armour_path_audit against obstacles in LINEAR MOTION.  obstacles [W][O][12] is every obstacle's pose at world time 0, velocity [W][O][3]
 * its constant velocity (finite), t_world [P] the world time of piece p's plan time 0 (finite): at world time w obstacle o is its zonotope
 * translated by v_o w.  Pieces, v_j, S, the midpoints t_s and the sub-interval half width half = (tb - ta) / (2S) are the static audit's
 * (armour_path_audit_items stays valid); verdicts, t_hit (a PLAN time), clearance and ms as there.
 * For item (p, s) and obstacle o, with tau = t_world[p] + t_s:
 * Sample test (exact).  The node rule's pair test of link box l against the staged obstacle o with the box centre x replaced by x - v_o tau
 *   (component-wise x[i] - v[i] * tau): the obstacle at its pose of world time tau.
 * Tube test (conservative).  The same shifted centre, and every half-size of link l enlarged by r_l + |v_o|_2 half, with
 *   |v_o|_2 = sqrt((v0^2 + v1^2) + v2^2) computed once per obstacle when it is staged.
 * Soundness.  Inside the sub-interval the obstacle is displaced from its midpoint pose by at most |v_o| half.  A meets B + d exactly when
 * A - d meets B, so testing the link box shifted by -v_o tau against the obstacle at its pose of time 0 is testing the box against the
 * obstacle at tau, and a displacement d of the obstacle with |d| <= rho is a displacement -d of the box; a box whose half-sizes grow by rho
 * contains the box (+) a ball of radius rho.  So if the box with half-sizes h_l + r_l + |v_o| half about the shifted midpoint centre is
 * separated from obstacle o, no configuration within e of the plan touches the obstacle at any time of the sub-interval (the static argument
 * supplies r_l).  Monotonicity carries over: the shift is the same in both tests and only the half-sizes grow, so a separated tube test still
 * implies a separated sample test bit for bit.  With zero velocities the results are armour_path_audit's bit for bit, for any t_world.
 * The device stages RM_OBS_STRIDE + 4 doubles per obstacle (the static 27, then v and |v|): 248 B of LDS each. */
int armour_path_audit_moving(const ArmourRobot* robot, int32_t W, int32_t O, const double* obstacles, const double* velocity, int32_t P,
                             const int32_t* world_of_piece, const double* t_world, const double* q0, const double* qd0, const double* qdd0,
                             const double* k, const double* k_range, double duration, const double* ta, const double* tb, const double* tube,
                             double step, int32_t* verdict, double* t_hit, double* clearance, double* ms);
/* the same rule by the same functions in a host loop (for tests; runs without a GPU) */
int armour_path_audit_moving_host(const ArmourRobot* robot, int32_t W, int32_t O, const double* obstacles, const double* velocity, int32_t P,
                                  const int32_t* world_of_piece, const double* t_world, const double* q0, const double* qd0, const double* qdd0,
                                  const double* k, const double* k_range, double duration, const double* ta, const double* tb, const double* tube,
                                  double step, int32_t* verdict, double* t_hit, double* clearance);
/* items [P] = S of every piece: the work items an audit at `step` takes (host arithmetic) */
int armour_path_audit_items(const ArmourRobot* robot, int32_t P, const double* q0, const double* qd0, const double* qdd0, const double* k,
                            const double* k_range, double duration, const double* ta, const double* tb, double step, int64_t* items);

/* ---- self-collision checks: the arm's link boxes against each other (self_check.hip) ---- */
/* The other half of the reference's collision flag (KSI/simulator_armtd.m ORs a self-intersection check into every collision check): is a
 * configuration, a roadmap edge or an executed plan piece free of collisions of the arm with itself?
 *
 * Boxes.  Link l at q is the node rule's box (above): the same frames, c_l and h_l.
 * Pair table.  pairs [J][J] uint8 (J = num_joints), only a < b is read; NULL is the default, every pair with b - a >= 2 (adjacent links'
 * bounding boxes always overlap).  A link whose half-sizes are all zero is never tested.  shrink [J][J] doubles, finite and >= 0, only
 * a < b is read; NULL is zeros.
 * Pair rule (exact for the boxes it is given).  Pair (a, b) is tested with box a as it is and box b with the half-sizes
 *   s_b = max(h_b - shrink_ab, 0) + r_ab          (r_ab = 0 for a configuration; the motion bound below otherwise),
 * d = x_b - x_a the centres' difference, u_ai / u_bk the boxes' unit axes.  The 15 axes m are the 3 axes of a, the 3 of b and the 9 cross
 * products u_ai x u_bk; a cross product with |m|^2 <= 1e-18 (the axes are unit: the sine of their angle <= 1e-9) is skipped, as in the
 * node rule.  value(m) = (|m.d| - sum_i s_ai |m.u_ai| - sum_k s_bk |m.u_bk|) / |m|, where a box's own axis contributes its own half-size
 * alone (its axes are orthonormal) and a cross product's two parents contribute nothing.
 *   pair clearance = max over the used axes of value;  configuration clearance = min over the listed pairs (+inf with none);
 *   SELF-FREE iff clearance > 0.  worst_pair = a J + b of the first pair (a, then b ascending) that attains the minimum.
 * Verdict mode (no clearance asked for) reads only the signs of the numerators, leaves a pair at its first separating axis and the
 * configuration at its first colliding pair; worst_pair is then that pair, or -1 when the configuration is free.
 *
 * Motion bound (relative).  The pose of link b in the frame of link a depends only on joints a+1 .. b: joints <= a move the pair rigidly,
 * and the test above is invariant under a rigid motion of both boxes.  Where every joint j stays within delta_j of a midpoint value,
 *   r_ab = sum over actuated j in a+1..b of rho_{j,b} delta_j,       rho_{j,l} the edge rule's (above).
 * Soundness: the edge rule's argument carried out in frame a.  Hold joints <= a at any value; turn joints a+1..b from their midpoint
 * values one at a time.  Turning joint j by theta turns every point of link b about an axis through p_j, which moves it by at most
 * rho_{j,b} theta -- in frame a as in the world, the two differ by a rigid motion.  So, seen from box a, every point of link b stays
 * within r_ab of its midpoint position, i.e. inside the midpoint box with half-sizes + r_ab, while box a does not move at all.  If the
 * enlarged box b is separated from box a at the midpoint, the two boxes are separated for every such configuration.  Only box b grows.
 *   Edge sub-segment s of S (the roadmap's S and midpoint):  delta_j = |D_j| / (2S).
 *   Audit sub-interval s of S (the path audit's S, midpoint and v_j):  delta_j = v_j (tb - ta) / (2S) + e_j.
 * A numerator is monotone in the half-sizes in floating point too, so an item whose enlarged test separates has a separated exact test.
 * Calibration.  sum_k |m.u_k| >= |m| for the axes of a box, so shrinking box b by d raises every axis value by at least d (until a
 * half-size reaches 0).  A pair that penetrates by p (clearance -p) at a configuration known to be harmless -- the boxes are coarser
 * than the arm -- is cleared there by shrink_ab = p + margin.
 *
 * Device.  One lane per (item, first link a); the lane runs the chain once, keeps box a and tests every listed b as the chain reaches
 * it.  Verdict bytes start at 1 and a colliding lane stores 0; clearances and worst pairs are merged on the host.  fp64 throughout.
 * Every entry has a _host twin that runs the same functions in a loop and needs no device. */
/* pairs [J][J] = the default table (1 where b - a >= 2) */
int armour_self_pairs_default(const ArmourRobot* robot, uint8_t* pairs);
/* q [N][n].  Outputs, each may be NULL: free [N] (0/1), clearance [N] (asking for it switches the early exits off), worst_pair [N],
 * ms = device time of the launch.  ARMOUR_EINVAL on a bad argument, before the device is touched. */
int armour_self_check(const ArmourRobot* robot, const uint8_t* pairs, const double* shrink, int32_t N, const double* q, uint8_t* free_,
                      double* clearance, int32_t* worst_pair, double* ms);
int armour_self_check_host(const ArmourRobot* robot, const uint8_t* pairs, const double* shrink, int32_t N, const double* q, uint8_t* free_,
                           double* clearance, int32_t* worst_pair);
/* The self masks of a roadmap, world-independent: one launch over (node | edge sub-segment, first link), once per roadmap.  An edge is
 * SELF-FREE iff every listed pair's enlarged test separates on every sub-segment, so no configuration on it self-collides and its
 * endpoints are self-free.  node_free [N], edge_free [E], node_clearance [N], ms: each may be NULL.  The handle keeps the masks and the
 * table for armour_roadmap_plan. */
int armour_roadmap_check_self(ArmourRoadmap* rm, const uint8_t* pairs, const double* shrink, uint8_t* node_free, uint8_t* edge_free,
                              double* node_clearance, double* ms);
/* on != 0: armour_roadmap_plan takes a node or edge as free only if it is free in the world's mask AND the self mask, and the edges it
 * checks on the host (direct, start and goal connections) also pass the self edge rule; ARMOUR_ESTATE from the plan before a self check.
 * Default off: armour_roadmap_plan is unchanged. */
int armour_roadmap_use_self(ArmourRoadmap* rm, int32_t on);
/* the self edge rule in a host loop, for edges qa[e] -> qb[e] ([E][n]) that need no roadmap: continuous [n] (NULL: robot->continuous) */
int armour_self_edges_host(const ArmourRobot* robot, const uint8_t* continuous, double edge_step, const uint8_t* pairs, const double* shrink, int32_t E,
                           const double* qa, const double* qb, uint8_t* edge_free);
/* armour_path_audit without a world: pieces, windows, tube, step, sub-intervals and outputs as there.  Verdict per piece: 0 PROVED
 * SELF-FREE (every enlarged test separates), 1 PROVED SELF-HIT (an exact test at a midpoint collides; t_hit = the first such t_s),
 * 2 UNDECIDED (neither; not a finding).  clearance [P] = the minimum exact configuration clearance over the midpoints (+inf with no pair). */
int armour_path_audit_self(const ArmourRobot* robot, const uint8_t* pairs, const double* shrink, int32_t P, const double* q0, const double* qd0,
                           const double* qdd0, const double* k, const double* k_range, double duration, const double* ta, const double* tb,
                           const double* tube, double step, int32_t* verdict, double* t_hit, double* clearance, double* ms);
int armour_path_audit_self_host(const ArmourRobot* robot, const uint8_t* pairs, const double* shrink, int32_t P, const double* q0, const double* qd0,
                                const double* qdd0, const double* k, const double* k_range, double duration, const double* ta, const double* tb,
                                const double* tube, double step, int32_t* verdict, double* t_hit, double* clearance);

#ifdef __cplusplus
}
#endif
#endif

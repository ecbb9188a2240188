/*
 * mpb.h -- C-ABI of libmpb_hip.so: MI355X (gfx950) kernels for the batched trajectory-optimisation
 * inner loops of anindex/motion_planning_baselines (mp_baselines/planners).
 *
 * The reference has NO FFI of its own (it is pure Python/PyTorch): the seam is the
 * planners' Python methods.  Each entry point below replaces the body of the reference method(s)
 * cited next to it; the classes in motion_planning_baselines_amd/planners keep the reference's class / ctor /
 * optimize() / reset() surface and call these through ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous row-major fp32 unless stated otherwise
 *     (obtained from tensor.data_ptr() of a PyTorch-ROCm tensor); the library never allocates,
 *     frees or retains caller memory and keeps no state between calls (thread-safe);
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream; NULL = default);
 *     all work is enqueued asynchronously on it, nothing synchronises the device;
 *   - return value 0 = ok; non-zero = MPB_E_*; mpb_last_error() gives the message of the calling
 *     thread's last failure;
 *   - shapes: P particles, S samples per particle, B = P*S rollouts, H support points (horizon),
 *     D degrees of freedom, d = optimised state width (D if pos_only else 2D).
 *   - `geom` is the packed geometry word buffer (motion_planning_baselines_amd/geometry.py
 *     pack_geometry; layout: the table at the top of that module, in C as mpb_geom_layout.h): robot
 *     kinematics + collision spheres + obstacle spheres / boxes + hinge margin.  It stands in for the reference's external robot / field objects
 *     (cost_functions.py:50-52 robot.fk_map_collision, field_factor.py:39 field.compute_cost).
 */
#ifndef MPB_H
#define MPB_H

#include <stddef.h>
#include <stdint.h>

/* the packed geometry buffer in numbers (generated from geometry.py): header word indices MPB_GW_*, geometry versions, robot
 * kinds, MPB_MAX_DOF / MPB_MAX_FIELDS and the grid limits, the cell-word fields, MPB_GEOM_FLAG_* */
#include "mpb_geom_layout.h"
#include "mpb_rrt_layout.h"
/* the packed self-collision buffer in numbers (generated from self_layout.py): header word indices MPB_SW_*, MPB_SELF_* */
#include "mpb_self_layout.h"
/* the packed SDF-grid buffer in numbers (generated from sdf_layout.py): header word indices MPB_DW_*, MPB_SDF_* */
#include "mpb_sdf_layout.h"
/* the packed triangle-mesh buffer in numbers (generated from mesh_layout.py): header word indices MPB_MW_*, record words MPB_TRI_*,
 * feature codes MPB_FEAT_*, MPB_MESH_* */
#include "mpb_mesh_layout.h"
/* the packed moving-obstacle buffer in numbers (generated from moving_layout.py): header word indices MPB_VW_*, MPB_MOVING_* */
#include "mpb_moving_layout.h"
/* the workspace and decision log of the space-time RRT-Connect in numbers (generated from strrt_layout.py): statuses MPB_STRRT_*, global
 * word indices MPB_STG_*, header word indices MPB_STH_*, log record words MPB_STL_* */
#include "mpb_strrt_layout.h"
/* path timing among moving obstacles in numbers (generated from path_timing_layout.py): statuses and limits MPB_PT_*, the LDS of a launch */
#include "mpb_path_timing_layout.h"
/* space-time shortcutting among moving obstacles in numbers (generated from st_shortcut_layout.py): statuses MPB_STS_*, log codes
 * MPB_STS_LOG_*, the Philox tag, the input gate's limit, limits, the LDS of a launch */
#include "mpb_st_shortcut_layout.h"
/* path certification by clearance bisection in numbers (generated from certify_layout.py): statuses MPB_CERT_*, the interval word, limits,
 * the reach buffer's header, the default slack */
#include "mpb_certify_layout.h"
/* space-time certification among moving obstacles in numbers (generated from st_certify_layout.py): MPB_STC_NOT_VALID, the words of a
 * trajectory's outputs, MPB_STC_NO_OBSTACLE, the default slack */
#include "mpb_st_certify_layout.h"
/* linear segments with parabolic blends in numbers (generated from blend_layout.py): statuses MPB_BLEND_*, the default sweep limit */
#include "mpb_blend_layout.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPB_OK 0
#define MPB_E_INVALID 1     /* bad argument (null pointer, shape out of range, bad geometry header) */
#define MPB_E_UNSUPPORTED 2 /* valid request this build cannot serve (e.g. H too large for LDS) */
#define MPB_E_HIP 3         /* a HIP runtime call failed; see mpb_last_error() */

#define MPB_MAX_H 256

/* ABI version in the low 16 bits (MPB_ABI_VERSION: bumped whenever a signature of this header changes positionally or a call that
 * used to be accepted is now refused; a binding must refuse a library that reports another number); bit 30 set = a tuning build
 * (compiled with wrong-result timing switches: never a product library).
 * Changes:  4 (round 4)  workspace header of the persistent STOMP kernels 64 -> 1 280 bytes; device-noise streams of STOMP / MPPI
 *                        changed (Philox4x32-7, 23-bit Box-Muller): not reproducible across 3 -> 4;
 *           5 (round 5)  geometry buffers are version 6 (broad-phase grid on a lattice through the origin, header word 31; a
 *                        version-5 buffer is refused by mpb_geom_check); the STOMP entry points refuse pointers that are not
 *                        16-byte aligned; a model-tagged geometry must keep margin + radii below 1 m; mpb_gpmp2_solve applies the
 *                        collision factors by Sherman-Morrison beyond a precision ratio of 1e7 (more accurate results there);
 *           6 (round 6)  mpb_gpmp2_workspace_bytes and mpb_stomp_workspace_bytes return MORE (the low-rank form of the GPMP2 solve keeps
 *                        its tables, right-hand sides and steps in the workspace; the STOMP workspace also fits the generalised persistent
 *                        kernel at H = 64, which serves list-grid scenes): a workspace sized by an older library is too small;
 *                        geometry buffers of version 7 (LIST broad-phase grid, per field) are accepted next to version 6;
 *                        MPB_MAX_DOF 8 -> 12; mpb_gpmp2_solve takes the low-rank form wherever n_fields (H - 1) <= 127 (same
 *                        results to the solver's fp64 rounding);
 *           7            batched RRT-Connect (mpb_rrt_connect_*) and mpb_collision_check added; nothing else changed.  ABI 7 now
 *                        also carries batched RRT* / informed RRT* (mpb_rrt_star_*): additive, no existing signature moved.
 *                        mpb_mppi_plan (how mpb_mppi_step would launch a shape) added the same way: additive; so was
 *                        mpb_traj_collision_stats (validation of a trajectory batch), and the self-collision field
 *                        (mpb_self_check, mpb_self_invalidate, mpb_self_collision_eval / _grad / _check).  So was the SDF-grid
 *                        field (mpb_sdf_grid_check, _invalidate, _build, _sample, _eval, _grad, _collision_check), and its build from
 *                        occupancy voxels (mpb_sdf_grid_build_occupancy).  So were the end-effector pose and batched inverse
 *                        kinematics (mpb_fk_ee_pose, mpb_ik_solve): additive.  So was the
 *                        end-effector pose cost (mpb_ee_cost_eval, mpb_ee_cost_grad), and the SDF grid's build from triangle
 *                        meshes (mpb_mesh_check, mpb_sdf_grid_build_mesh), path shortcutting and the roadmap planner, and
 *                        the time parameterisation under joint limits (mpb_traj_retime, mpb_traj_retime_sample), and Cartesian
 *                        end-effector moves (mpb_cartesian_path), and the moving-obstacle field (mpb_moving_check,
 *                        mpb_moving_invalidate, mpb_moving_collision_eval / _grad / _check), and the timing of geometric paths among
 *                        moving obstacles (mpb_path_time_plan), and space-time shortcutting (mpb_st_shortcut): additive.  So were
 *                        the clearance op and the path certifier (mpb_clearance, mpb_path_certify), and the world predicate and the
 *                        *_world entries (mpb_world_collision_check, mpb_rrt_connect_init_world / _run_world, mpb_path_shortcut_world,
 *                        mpb_traj_collision_stats_world).  So were the clearance of a timed trajectory's rows against a moving field
 *                        and the space-time certifier (mpb_moving_clearance, mpb_traj_certify_moving): additive.  So were linear
 *                        segments with parabolic blends (mpb_path_blend, mpb_path_blend_sample): additive. */
#define MPB_ABI_VERSION 7
#define MPB_VERSION_TUNING_BUILD 0x40000000
int mpb_version(void);
const char *mpb_last_error(void);

/* Validate a packed geometry buffer held in HOST memory (n_words 32-bit words). */
int mpb_geom_check(const float *geom_host, int n_words);
/* Properties of a (valid) packed geometry buffer, read from its HOST copy, that let a launcher pick a kernel
 * instantiation without touching device memory.  *flags is built from MPB_GEOM_FLAG_* of mpb_geom_layout.h (the values
 * are what they have been since the bits were introduced; bit 11 is unused):
 *   & MPB_GEOM_FLAG_MODEL_MASK   id of the compile-time robot model (csrc/mpb_model_*.h) EVERY chained field is tagged with
 *                                and every field has a usable grid of either format; 0 = generic table-driven kernels.
 *                                Only the generalised persistent STOMP kernel runs the model on list grids: every other
 *                                consumer requires MPB_GEOM_FLAG_ALL_GRIDS beside it;
 *   MPB_GEOM_FLAG_ALL_GRIDS      every chained field has a usable COMPACT broad-phase grid (geometry version 6, at most
 *                                MPB_GRID_MAX_SPH obstacle spheres): what the persistent STOMP kernels and the cost-only
 *                                model kernels need;
 *   MPB_GEOM_FLAG_POINT_SMALL    point robot with ONE field of at most 32 spheres and 8 boxes (CHOMP's
 *                                four-lanes-per-waypoint kernel keeps such an obstacle set in registers);
 *   MPB_GEOM_FLAG_POINT          point robot;
 *   MPB_GEOM_FLAG_ONE_FIELD      ONE field, no chain (MPPI's LDS grid, the persistent STOMP kernels' one-field instantiations);
 *   MPB_GEOM_FLAG_ALL_LISTS      (round 6) every chained field carries a LIST grid (geometry version 7: a field with more
 *                                obstacle spheres than a compact grid serves -- up to MPB_LIST_MAX_SPH spheres +
 *                                MPB_LIST_MAX_BOX boxes, any number of candidates per cell, boxes culled like spheres;
 *                                MPB_GEOM_FLAG_ALL_GRIDS is then clear): the generalised persistent STOMP kernel takes such a
 *                                geometry up to H = 64 (csrc/mpb_stomp_fused_hx.hip, LIST), every other kernel walks such a
 *                                field exhaustively;
 *   >> MPB_GEOM_FLAG_CELLS_SHIFT & MPB_GEOM_FLAG_CELLS_MASK   cells of the largest broad-phase grid of the chain when ALL_GRIDS or
 *                                ALL_LISTS is set (what a kernel that stages the grid in LDS has to reserve).
 * Entry points that take `geom_flags` expect the value computed from the host copy of the very buffer `geom` points to
 * (0 is always valid); a kernel re-checks the tag and the one-field promise against the device header and writes NaN
 * costs if they disagree. */
int mpb_geom_flags(const float *geom_host, int n_words, int *flags);

/* ---------------------------------------------------------------------------------------------
 * Collision cost  -- replaces CostCollision.eval (costs/cost_functions.py:171-189) over
 * get_q_pos_vel_and_fk_map (:41-53) + FieldFactor.get_error (costs/factors/field_factor.py:17-39):
 *   out[b] = weight * (k_sigma * sum_{h >= h_begin} field_cost(q[b,h,:D]))       (h_begin = 1: Q5)
 * trajs (B,H,d); out (B).
 * mpb_cost_collision_grad additionally writes grad (B,H,d) = d out[b] / d trajs[b] (the quantity the
 * reference obtains by autograd: chomp.py:139, field_factor.py:54); velocity channels get 0.
 * per_waypoint (B,H) optional (may be NULL): un-scaled field cost of every waypoint (0 for h < h_begin).
 * geom_flags = mpb_geom_flags(host copy of geom) lets the gradient evaluators pick the compile-time robot model's kernel
 * (same bits as the table-driven walk, fewer instructions and registers); 0 is always valid (table-driven walk).
 * ------------------------------------------------------------------------------------------- */
int mpb_cost_collision_eval(const float *trajs, const float *geom, float *out, float *per_waypoint,
                            int B, int H, int d, int h_begin, float k_sigma, float weight, void *stream);
int mpb_cost_collision_grad(const float *trajs, const float *geom, int geom_flags, float *out, float *grad,
                            int B, int H, int d, int h_begin, float k_sigma, float weight, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Trajectory-only cost terms -- replaces the eval() of CostGP (costs/cost_functions.py:271-289),
 * CostGPTrajectory (:344-354), CostGPTrajectoryPositionOnlyWrapper (:365-368), CostSmoothnessCHOMP
 * (:384-387), CostJointLimits (:406-426) and CostGoalPrior (:523-536); any subset in one pass over the
 * batch (what CostComposite.eval, :70-87, sums term by term):
 *   out[b] (+)= k_gp    * sum_t e_t^T ([[12/dt^3,-6/dt^2],[-6/dt^2,4/dt]] (x) I) e_t, e_t = x_{t+1} - Phi x_t
 *            + k_start * |start_state - x_0|^2            (UnaryFactor, K = I/sigma^2 folded into k_*)
 *            + k_goal  * |goal_states[b / trajs_per_goal] - x_{H-1}|^2
 *            + k_smooth* sum_cols x^T R x, R = CHOMP._get_R_mat(dt, H) (chomp.py:81-101)
 *   *jl_total   = k_jlim * sum over the WHOLE batch of squared joint-limit violations beyond
 *                 q_min + jl_eps / q_max - jl_eps (the reference's `.sum(-1)` of a 1-D gather is a scalar);
 *                 broadcast_jlim != 0 also adds it to every out[b] (what the composite's `+=` does).
 * k_* = composite weight / sigma^2 of the term.  trajs (B,H,d) with d == 2*n_dof, or d == n_dof with
 * MPB_TERM_VEL_FD (velocities = central differences, zero end rows) for the GP term / any d for
 * SMOOTH / d >= n_dof for JLIM.  start_state (2*n_dof), goal_states (G, 2*n_dof), q_min/q_max (n_dof),
 * jl_total: one fp64 word, all device memory; pointers of disabled terms may be NULL.
 * accumulate != 0 adds onto the existing out[b] (e.g. the collision costs mpb_stomp_sample wrote).
 * ------------------------------------------------------------------------------------------- */
#define MPB_TERM_GP 1u
#define MPB_TERM_START 2u
#define MPB_TERM_GOAL 4u
#define MPB_TERM_SMOOTH 8u
#define MPB_TERM_JLIM 16u
#define MPB_TERM_VEL_FD 32u
#define MPB_TERM_ALL 63u
int mpb_cost_terms_eval(const float *trajs, float *out, double *jl_total, const float *start_state,
                        const float *goal_states, const float *q_min, const float *q_max,
                        int B, int H, int d, int n_dof, int trajs_per_goal, uint32_t flags, float dt,
                        float k_gp, float k_start, float k_goal, float k_smooth, float k_jlim, float jl_eps,
                        int accumulate, int broadcast_jlim, void *stream);
/* Analytic gradient of the same terms -- what the reference obtains by autograd through CostComposite.eval when CHOMP
 * differentiates costs.sum() (chomp.py:135-139) -- and, with apply != 0, CHOMP's update in the same pass (:141-147):
 *   g = grad_in (may be NULL; e.g. mpb_cost_collision_grad's output) + d/dx [enabled terms, k_* as in
 *       mpb_cost_terms_eval; the joint-limit term times jl_scale: its batch-global scalar sits in EVERY trajectory's
 *       cost, so the gradient of costs.sum() carries the global batch size] + prior_bw * (R + R^T) x (CHOMP's
 *       smoothness prior, prior_bw = B_global * weight_prior_cost: quirk Q3; R (H,H), only its tridiagonal band is read)
 *   apply == 0: grad_out (B,H,d) = g;  apply != 0: trajs -= lr * mask(clamp(g, -grad_clip, grad_clip)) in place,
 *   the mask zeroing rows 0 and H-1.  grad_in / grad_out may alias. */
int mpb_cost_terms_grad(float *trajs, const float *grad_in, float *grad_out, const float *R,
                        const float *start_state, const float *goal_states, const float *q_min, const float *q_max,
                        int B, int H, int d, int n_dof, int trajs_per_goal, uint32_t flags, float dt,
                        float k_gp, float k_start, float k_goal, float k_smooth, float k_jlim, float jl_eps,
                        float jl_scale, float prior_bw, float lr, float grad_clip, int apply, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Trajectory utilities either side of the loop (all external to the reference: torch_robotics; build-defined).
 *   mpb_traj_interpolate       -- interpolate_points_v1 (call site cost_functions.py:118): n_interp evenly
 *                                 spaced points inserted between consecutive waypoints, linear in joint
 *                                 space: trajs (B,H,d) -> out (B,(H-1)*(n_interp+1)+1,d).
 *   mpb_traj_finite_difference -- finite_difference_vector(method='central') + the concatenation of
 *                                 OptimizationPlanner._get_traj (base.py:204-213): pos (B,H,D) ->
 *                                 out (B,H,2D) = [pos, (pos_{t+1}-pos_{t-1})/(2 dt)], zero end velocities.
 *   mpb_traj_resample          -- the warm start of HybridPlanner.optimize (hybrid_planner.py:42-66, over the
 *                                 external smoothen_trajectory / tensor_linspace_v1): N polylines of
 *                                 lengths[n] <= Lmax waypoints (paths (N,Lmax,D), rows beyond the length
 *                                 ignored and never read; a length outside 1 .. Lmax is clamped into it)
 *                                 -> out (N,H,2D): H points uniform in arc length, linear in between,
 *                                 velocity = (last - first)/((H-1) dt) on interior points, 0 at ends.
 * ------------------------------------------------------------------------------------------- */
int mpb_traj_resample(const float *paths, const int *lengths, float *out, int N, int Lmax, int H, int D, float dt,
                      void *stream);
int mpb_traj_interpolate(const float *trajs, float *out, int B, int H, int d, int n_interp, void *stream);
/* GPFactor.get_error (costs/factors/gp_factor.py:52-56): err[b,t] = x[b,t+1] - Phi x[b,t]; x (B,H,2D) -> out (B,H-1,2D) */
int mpb_gp_factor_error(const float *x, float *out, int B, int H, int D, float dt, void *stream);
int mpb_traj_finite_difference(const float *pos, float *out, int B, int H, int D, float dt, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The robot / field API the reference's cost layer consumes (provider in the reference: torch_robotics), as separate
 * device ops with vector-Jacobian products, so that the UNMODIFIED reference cost classes can run on this package's
 * robot / field objects and torch.autograd can differentiate through them (field_factor.py:54):
 *   mpb_fk_collision_points      robot.fk_map_collision (call site cost_functions.py:52): q (B,H,d) -> pts (B,H,L,3)
 *   mpb_fk_collision_points_vjp  grad_q (B,H,n_dof) = J^T grad_pts
 *   mpb_field_cost_points        field.compute_cost (call sites field_factor.py:39,52): pts (B,H,L,3) -> cost (B,H)
 *                                = sum_l relu(margin + r_l - min_o sdf_o(pts_l))   (first field of `geom`)
 *   mpb_field_cost_points_vjp    grad_pts (B,H,L,3) = grad_cost (B,H) * d cost / d pts
 * The planners never call these (they use the fused evaluators); L = number of collision spheres of the robot.
 * ------------------------------------------------------------------------------------------- */
int mpb_fk_collision_points(const float *q, const float *geom, float *pts, int B, int H, int d, void *stream);
int mpb_fk_collision_points_vjp(const float *q, const float *geom, const float *grad_pts, float *grad_q,
                                int B, int H, int d, void *stream);
int mpb_field_cost_points(const float *pts, const float *geom, float *cost, int B, int H, void *stream);
int mpb_field_cost_points_vjp(const float *pts, const float *geom, const float *grad_cost, float *grad_pts,
                              int B, int H, void *stream);

/* ---------------------------------------------------------------------------------------------
 * STOMP -- replaces STOMP._run_optimization's loop body (stomp.py:150-160):
 *   sample (stomp.py:97-108 + MultivariateNormal.rsample), _get_costs (base.py:218-223) with the
 *   collision cost above, _calc_sample_weights (stomp.py:219-220), _update_distribution (:199-211).
 *
 * means (P,H,d) in/out, updated in place n_iters times.
 * eps: NULL -> standard normals are generated on the device (Philox4x32, 7 rounds, keyed by `seed`,
 *      counter = (particle_offset + p, s, (channel, waypoint group, call), iter0 + i); Box-Muller on 23-bit uniforms, a
 *      drawn normal carries 16 significant bits -- csrc/mpb_stomp_noise.h; result independent of sharding and of the
 *      kernel that serves the call);
 *      else (n_iters, S, d, P, H): pre-drawn standard normals in the reference's draw order
 *      (one MultivariateNormal.sample((S,d)) of batch shape (P,) and event shape (H,) per iteration).
 * samples (P,S,H,d), costs (P,S), weights (P,S): outputs of the LAST iteration (all required).
 *      A persistent launch (mpb_stomp_run*) writes them for its last iteration ONLY -- once per launch, never per iteration;
 *      with n_iters = 0 they are not written at all.
 * Alignment: means, eps, samples, L, Sigma, geom (and the workspace / means_copy of mpb_stomp_run*) must be 16-byte aligned --
 *      the kernels move them as 16-byte vectors; a pointer that is not is refused with MPB_E_INVALID (allocations of hipMalloc /
 *      PyTorch-ROCm are 256-byte aligned; a VIEW at an odd element offset is what trips this).
 * L (H,H): scale_tril of the noise distribution, Sigma (H,H) = inverse(R): constants the host
 *      computes exactly as the reference does (stomp.py:63-64, :88-95) -- SURVEY.md H2.
 * mpb_stomp_step runs the fused path (sample+cost kernel, update kernel per iteration).  Everything is
 * enqueued asynchronously; only for n_iters > 256 (and never under stream capture) the call blocks on its
 * own events so that at most 256 iterations are queued ahead of the GPU.
 * mpb_stomp_update accepts Sigma == NULL (update without the covariance product, used by StochGPMP).  Its envelope:
 *      S >= 1, 3 <= H <= MPB_MAX_H, 1 <= d <= 2 * MPB_MAX_DOF (the update kernels have no channel tile: StochGPMP's positions
 *      + velocities of up to 12 joints; the sampling kernels keep d <= 16, one matrix-core tile), and its LDS within
 *      150 KB: S + 5 H d floats (plus H*H for lr*Sigma while that fits 64 KB) -- MPB_E_UNSUPPORTED beyond it.
 * mpb_stomp_sample / mpb_stomp_update expose the two halves (the two kernels of one iteration) so that
 * a caller-supplied cost callable (any Python cost on device tensors) can sit between them; with
 * geom + costs given, mpb_stomp_sample is exactly the first kernel of mpb_stomp_step.
 * ------------------------------------------------------------------------------------------- */
int mpb_stomp_step(float *means, const float *eps, float *samples, float *costs, float *weights,
                   const float *L, const float *Sigma, const float *geom, int geom_flags,
                   int P, int S, int H, int d, int D,
                   float k_sigma, float weight, float lr, float temperature,
                   int n_iters, uint64_t seed, uint32_t iter0, uint32_t particle_offset, void *stream);
/* Measurement aid for bench.py: the n_iters (1..1024) iterations of mpb_stomp_step with device noise, every kernel
 * launch carrying its own pair of HIP events on the dispatch (hipExtLaunchKernelGGL), then ONE stream synchronise.
 * Writes the average duration in ms of the sample+cost kernel and of the update kernel, measured in the loop they
 * run in (the per-kernel figure rocprofv3 --kernel-trace --stats reports for the same loop).  Host pointers. */
int mpb_stomp_step_profile(float *means, float *samples, float *costs, float *weights,
                           const float *L, const float *Sigma, const float *geom, int geom_flags,
                           int P, int S, int H, int d, int D,
                           float k_sigma, float weight, float lr, float temperature,
                           int n_iters, uint64_t seed, uint32_t iter0, uint32_t particle_offset, void *stream,
                           float *sample_kernel_ms, float *update_kernel_ms);
#define MPB_STOMP_WS_HEADER_BYTES 1280
/* The same loop as ONE persistent launch (csrc/mpb_stomp_fused.hip): a workgroup of 16 waves owns (particle, chunk of 16
 * samples) for all n_iters iterations -- constants, means and the iteration's samples stay in LDS, the partners of a
 * particle (S > 16) exchange their 3.6 KB partial sums through `workspace`; no per-iteration launch ramps or dispatch
 * gaps.  Same arguments and outputs as mpb_stomp_step plus the caller-allocated workspace (mpb_stomp_workspace_bytes;
 * its header, the first MPB_STOMP_WS_HEADER_BYTES, must be ZERO before the first call -- mpb_stomp_workspace_init -- and is
 * maintained by the library afterwards (ABI 4: 1 280 bytes, the counters the workgroups hit at start-up one cache line each; 64 before); the rest need not be initialised; one workspace serves one call at a time).  Served for H = 64, S <= 64,
 * grid-backed fields (geom_flags bit 8); any other call -- or workspace == NULL -- runs mpb_stomp_step
 * (mpb_stomp_run_path tells which, without launching).  The softmax is evaluated as exp(x - m) / z over per-chunk
 * partials, the same weights up to rounding.  When the particles are at least as many as the CUs (and 16 < S <= 32) one
 * workgroup per particle runs the samples as two batches of 16 instead -- no exchange, same bits (environment
 * MPB_STOMP_BATCHES = 1 / 2 forces a layout; a test aid).
 *
 * Failure contract.  The workgroups of a particle wait for each other's partial sums every iteration.  They are paired
 * by a ticket drawn when a workgroup STARTS (not by block index), so partners are always workgroups that started next to
 * each other and no dispatch order or co-residency is assumed; every wait is nevertheless bounded (2 s + 100 us per
 * iteration; MPB_STOMP_TIMEOUT_US overrides, a test aid).  A workgroup whose partner does not arrive in time -- the
 * device stopped starting this grid's workgroups for that long, e.g. another context holds every CU -- marks the call
 * LOST: every workgroup leaves, the means of the affected particles are not written, samples / costs / weights are
 * undefined.  The call still returns MPB_OK (it is asynchronous); the loss is reported
 *   - by mpb_stomp_run_status (reads the workspace header; synchronises the stream): 0 fine, 1 lost, 2 header not zeroed;
 *   - without synchronising, by mpb_stomp_run_checked's `status`: 8 words of pinned, device-mapped HOST memory
 *     (hipHostMalloc), zero before the first call: [0] = tag of the last call that has completed, [1] = tag of the last
 *     call that was lost (0: none), [2] = why (1 partner timed out, 2 header not zeroed), [4..5] / [6..7] = the device's
 *     100 MHz real-time counter when the launch's first unit started / when its last workgroup left (the launch's
 *     duration as the device saw it: a measurement aid that costs nothing); `tag_out` receives the tag
 *     of this call (0 when it ran the two-kernel loop, which cannot be lost).  The caller compares [1] with the tags it
 *     has issued whenever convenient -- planners/stomp.py raises at the next planner call.  Word [0] says the tag was
 *     PUBLISHED -- every workgroup's result stores are ordered before it (each wave drains its stores, a block barrier,
 *     then the release) -- not that the kernel has retired: a consumer on ANOTHER stream must still order itself behind
 *     the launch stream (event / stream wait); work on the launch stream and host reads after a stream / device
 *     synchronise are ordered as always.
 * means_copy (P,H,d) or NULL: a second destination for the final means, written by the same launch (the reference's
 * optimize() returns a CLONE of its means, base.py:204-213: this saves the dependent copy kernel).
 * Not capturable in a HIP graph (the per-call tag is drawn on the host). */
#define MPB_STOMP_PATH_TWO_KERNEL 0
#define MPB_STOMP_PATH_PERSISTENT_EXCHANGE 1   /* one workgroup per (particle, chunk of 16 samples), partials exchanged */
#define MPB_STOMP_PATH_PERSISTENT 2            /* one workgroup per particle (S <= 16, or two batches of 16), no exchange */
size_t mpb_stomp_workspace_bytes(int P, int S, int H, int d);
int mpb_stomp_workspace_init(float *workspace, size_t workspace_bytes, void *stream);
int mpb_stomp_run_path(int geom_flags, size_t workspace_bytes, int P, int S, int H, int d);
int mpb_stomp_run(float *means, const float *eps, float *samples, float *costs, float *weights,
                  const float *L, const float *Sigma, const float *geom, int geom_flags,
                  float *workspace, size_t workspace_bytes,
                  int P, int S, int H, int d, int D,
                  float k_sigma, float weight, float lr, float temperature,
                  int n_iters, uint64_t seed, uint32_t iter0, uint32_t particle_offset, void *stream);
int mpb_stomp_run_checked(float *means, const float *eps, float *samples, float *costs, float *weights,
                          const float *L, const float *Sigma, const float *geom, int geom_flags,
                          float *workspace, size_t workspace_bytes,
                          int P, int S, int H, int d, int D,
                          float k_sigma, float weight, float lr, float temperature,
                          int n_iters, uint64_t seed, uint32_t iter0, uint32_t particle_offset,
                          uint32_t *status, uint32_t *tag_out, float *means_copy, void *stream);
int mpb_stomp_run_status(const float *workspace, void *stream, int *timed_out);
/* Measurement aid (bench.py): mpb_stomp_run_checked with the persistent kernel's begin / end timestamps recorded on the
 * dispatch itself (what rocprofv3 --kernel-trace reports); synchronises the stream; *kernel_ms = the kernel's duration in
 * milliseconds (0 when the call ran the two-kernel loop). */
int mpb_stomp_run_timed(float *means, const float *eps, float *samples, float *costs, float *weights,
                        const float *L, const float *Sigma, const float *geom, int geom_flags,
                        float *workspace, size_t workspace_bytes,
                        int P, int S, int H, int d, int D,
                        float k_sigma, float weight, float lr, float temperature,
                        int n_iters, uint64_t seed, uint32_t iter0, uint32_t particle_offset,
                        uint32_t *status, uint32_t *tag_out, float *means_copy, void *stream, float *kernel_ms);
/* A persistent-launch call with everything but (n_iters, iter0, means_copy, stream) fixed, kept on the library's side (round 4):
 * for a binding whose foreign-function marshalling is not free (ctypes: ~3 us for the 28 arguments of mpb_stomp_run_checked,
 * a quarter of the host side of a call).  mpb_stomp_plan_create validates and copies the arguments (host memory only: one small
 * malloc, the one place the library allocates; device noise only, eps = NULL); mpb_stomp_plan_launch == mpb_stomp_run_checked on
 * them (same failure contract, same tag); mpb_stomp_plan_destroy frees the record.  The caller keeps every buffer alive. */
typedef struct mpb_stomp_plan_s mpb_stomp_plan;
int mpb_stomp_plan_create(mpb_stomp_plan **plan, float *means, float *samples, float *costs, float *weights,
                          const float *L, const float *Sigma, const float *geom, int geom_flags,
                          float *workspace, size_t workspace_bytes, int P, int S, int H, int d, int D,
                          float k_sigma, float weight, float lr, float temperature, uint64_t seed, uint32_t particle_offset,
                          uint32_t *status);
int mpb_stomp_plan_launch(mpb_stomp_plan *plan, int n_iters, uint32_t iter0, float *means_copy, void *stream, uint32_t *tag_out);
int mpb_stomp_plan_destroy(mpb_stomp_plan *plan);

int mpb_stomp_sample(const float *means, const float *eps, float *samples, const float *L,
                     const float *geom, int geom_flags, float *costs, /* geom, costs both NULL: sample only; both set: fused cost */
                     int P, int S, int H, int d, float k_sigma, float weight,
                     uint64_t seed, uint32_t iter, uint32_t particle_offset, void *stream);
int mpb_stomp_update(float *means, const float *samples, const float *costs, float *weights,
                     const float *Sigma, int P, int S, int H, int d, float lr, float temperature,
                     void *stream);

/* ---------------------------------------------------------------------------------------------
 * CHOMP -- replaces CHOMP._run_optimization's loop body (chomp.py:127-151) and _eval (:153-169):
 *   g = d/dx [ collision cost + w_prior * B_global * sum_c x_c^T R x_c ]   (quirk Q3: the batch-total
 *   smoothness scalar is added to every particle's cost and costs.sum() is differentiated, so the
 *   smoothness gradient carries the GLOBAL batch size), clamp to +-grad_clip, zero the two endpoint
 *   rows, x -= lr * g;  repeated n_iters times inside one launch.
 * means (B_local,H,d) in/out.  R (H,H): CHOMP._get_R_mat (chomp.py:81-101), computed by the host;
 * only its tridiagonal band is read.  costs_out (B_local) optional: collision cost (scaled) of the
 * iterate BEFORE the last update, without the smoothness scalar.
 * ------------------------------------------------------------------------------------------- */
int mpb_chomp_step(float *means, const float *R, const float *geom, int geom_flags, float *costs_out,
                   int B_local, int B_global, int H, int d, int D,
                   float k_sigma, float weight, float w_prior, float lr, float grad_clip,
                   int n_iters, void *stream);

/* ---------------------------------------------------------------------------------------------
 * GPMP2 -- replaces GPMP2._step (gpmp2.py:308-342): CostComposite.get_linear_system
 * (cost_functions.py:107-144 over CostGP :291-314, CostGoalPrior :538-554, CostCollision :191-231),
 * _get_grad_terms dense branch (gpmp2.py:355-368), get_torch_solve('cholesky') (:451-452) and the
 * update (:339), WITHOUT materialising the dense (A,b,K): the normal equations A^T K A are
 * block-tridiagonal with 2D x 2D blocks and are assembled and solved per particle by block Cholesky.
 * Internal arithmetic is fp64 (weights reach 1/sigma^2 = 1e10); x is stored in fp32.
 *
 * x (B,H,2D) in/out; start (B,2D), goal (B,2D) per-particle states (zero velocities appended by the
 * host; the reference's single start / goal is broadcast by the caller).
 * workspace: caller-allocated device scratch of mpb_gpmp2_workspace_bytes(B,H,D) bytes, 256-byte
 * aligned (collision Jacobians, the diagonal sums and the per-step elimination factors).
 *
 * One iteration = linearize -> [diag] -> solve:
 *   mpb_gpmp2_linearize : collision cost c_t and Jacobian h_t = -dc_t/dq of every waypoint (FieldFactor
 *                         get_error(calc_jacobian=True), field_factor.py:41-57) into the workspace.
 *                         n_interp > 0 (CostComposite.get_linear_system(n_interpolated_points),
 *                         cost_functions.py:115-119): h_t = -d/dq_t of the summed cost of the trajectory
 *                         with n_interp points inserted per segment (see mpb_traj_interpolate); c_t unchanged;
 *   mpb_gpmp2_diag      : LOCAL SUM over the B particles of diag(A^T K A) (H*2D fp64) -- quirk Q9: the
 *                         trust-region damping uses the BATCH MEAN of that diagonal (gpmp2.py:361-367).
 *                         diag_sum_out NULL: kept in the workspace.  When sharded, the host all-reduces
 *                         the sums and passes diag_mean = sum / B_global to mpb_gpmp2_solve;
 *   mpb_gpmp2_solve     : assemble + solve + x += step_size * dtheta.  Two forms of the same fp64 solve: the LOW-RANK form
 *                         (round 6, csrc/mpb_gpmp2_lr.hip: priors + GP blocks + damping are shared by all particles and decouple
 *                         over the joints -- factored once per call --, the collision factors enter through a dense SPD system
 *                         over each particle's ACTIVE rows; as accurate as dense fp64 Cholesky at every precision ratio) wherever
 *                         n_fields * (H - 1) <= 127, and the block-tridiagonal elimination (csrc/mpb_gpmp2.hip) otherwise (D <= 8
 *                         only: a 2D x 2D block must fit its 16 x 16 tile).  MPB_GPMP2_FORM = lr / block (environment, read per
 *                         call) forces one; MPB_GPMP2_SM set means the block form.
 *                         trust_region == 0: damping delta * I (diag_mean ignored);
 *                         else delta * diag_mean (diag_mean NULL: the LOCAL mean mpb_gpmp2_diag leaves in the workspace
 *                         when it is called without diag_sum_out, as mpb_gpmp2_step does).
 *                         costs_out (B) optional: b^T K b of the iterate BEFORE the update (gpmp2.py:493-495).
 *   mpb_gpmp2_step      : n_iters full iterations on one GPU (mean over the local B).
 * Accuracy: the elimination forms W_t = S_t^-1 explicitly (blocked Gauss-Jordan, fp64).  With the rank-1 collision term
 * ASSEMBLED into S_t that resolves its stiff direction to kappa^2 u where a Cholesky factorisation gives kappa u: step error
 * against the dense fp64 solution refined in long double 5e-8 at a ratio (sigma_gp / sigma_coll)^2 of the collision to the GP
 * precision of 1e6 (the reference's defaults), <= 2.3e-6 at 1e8, 8e-3 at 1e10 (ABI <= 4 as released in round 4).  Since round 5
 * mpb_gpmp2_solve applies the collision factors by SHERMAN-MORRISON on the inverse of the well-conditioned rest whenever
 * (sigma_gp / sigma_coll)^2 * n_fields > 1e7 (csrc/mpb_gpmp2.hip, template flag SM; +7.5 % on the solve): measured 3e-8 .. 7e-8 at
 * 1e8 and 1e10 (one / two fields, trust region on / off, interpolated Jacobian), 1.2e-5 at 1e12 where the dense fp64 Cholesky
 * is itself at ~1e-6 -- no range to keep to.  MPB_GPMP2_SM = 0 / 1 (environment) forces a form; the start / goal precisions
 * (1e10 .. 1e12 tested) do not matter.
 * Alignment: x and geom 16-byte aligned, workspace 256-byte aligned (rows are moved as 8- / 16-byte pieces); a pointer
 * that is not is refused with MPB_E_INVALID (allocations of hipMalloc / PyTorch-ROCm are 256-byte aligned; a VIEW with a
 * storage offset may not be).
 * sigma_goal <= 0 means "no goal factor" (precision 0: GPMP2 without goals, gpmp2.py:62-78) -- an infinite sigma is not a
 * valid argument (the library is built with -ffinite-math-only).
 * n_fields = number of collision fields chained in `geom` (1..4; see mpb_geom_check): the reference stacks one
 * block of H-1 collision rows per field (gpmp2.py:70-78, cost_functions.py:107-144), the workspace keeps one
 * (h_t, c_t) set per field and the solve sums their rank-1 terms.
 * ------------------------------------------------------------------------------------------- */
size_t mpb_gpmp2_workspace_bytes(int B, int H, int D);
int mpb_gpmp2_linearize(const float *x, const float *geom, int geom_flags, void *workspace, int B, int H, int D,
                        int n_interp, void *stream);
int mpb_gpmp2_diag(void *workspace, double *diag_sum_out, int B, int H, int D, int n_fields, float dt,
                   float sigma_start, float sigma_gp, float sigma_goal, float sigma_coll, void *stream);
int mpb_gpmp2_solve(float *x, const float *start, const float *goal, const double *diag_mean, void *workspace,
                    float *costs_out, int B, int H, int D, int n_fields, float dt,
                    float sigma_start, float sigma_gp, float sigma_goal, float sigma_coll,
                    float delta, int trust_region, float step_size, void *stream);
int mpb_gpmp2_step(float *x, const float *start, const float *goal, const float *geom, int geom_flags, void *workspace,
                   float *costs_out, int B, int H, int D, float dt,
                   float sigma_start, float sigma_gp, float sigma_goal, float sigma_coll,
                   float delta, int trust_region, float step_size, int n_iters, int n_interp, int n_fields,
                   void *stream);

/* ---------------------------------------------------------------------------------------------
 * MPPI -- replaces MPPI.optimize's loop body (mppi.py:145-152): ControlTrajectoryGaussian.sample
 * (priors/gaussian.py:276-298), get_state_trajectories_rollout (mppi.py:190-210) over
 * PointParticleDynamics.dynamics (dynamics/point.py:102-140, deterministic), traj_cost (:154-226),
 * the importance-sampling term (mppi.py:125-128) and update_controller (:72-86).
 * One problem per workgroup; NP independent problems per launch (the reference class is NP = 1);
 * all n_iters iterations inside one launch.
 *
 * mean (NP,T,c) in/out; eps NULL -> standard normals generated on the device (since ABI 4: Philox4x32 with 7 rounds keyed by
 * `seed`, counter = (problem, sample, (t / 4) | dim << 16, iter0 + i), one call per four consecutive time steps; Box-Muller
 * on the top 23 bits of each word, so |n| <= sqrt(2 ln 2^23) = 5.65; ABI 3 drew Philox4x32-10 with 24-bit uniforms: the
 * device-noise streams of STOMP and MPPI are NOT reproducible across ABI 3 -> 4; mpb_debug_mppi_normals of include/mpb_debug.h
 * returns the stream), else (n_iters,NP,c,S,T) standard normals (per
 * control dimension, in the reference's draw order); scale_tril, cov_inv (c,T,T); state0 (NP,c);
 * goal (NP,c); ctrl_min / ctrl_max (c); discount (T); c_weights = {pos, vel, ctrl, pos_T};
 * control_type 0 = velocity (state_dim = c); 1 = acceleration is MPB_E_UNSUPPORTED (the reference's
 * acceleration mode slices an empty tensor, point.py:114-118, and cannot run).
 * geom optional (NULL = no collision term); geom_flags = mpb_geom_flags(host copy of geom) (0 is always valid): with a
 * single grid-backed field the collision cost of a rollout goes through the broad-phase grid (staged in LDS: one
 * candidate look-up per waypoint instead of the exhaustive obstacle loop; same bits).  With geom, the reference's quirk Q6 is reproduced:
 * the per-sample collision costs are summed into ONE scalar that is added to every sample's cost.
 * Outputs of the last iteration: controls (NP,S,T,c), states (NP,S,T,c), costs (NP,S), weights (NP,S).
 * best_cost (NP) in/out + best_states (NP,T,c) out, both or neither (NULL): MPPI._save_best
 * (mppi.py:164-168, called every iteration, mppi.py:148): whenever an iteration's cheapest sample (first
 * index on ties) beats best_cost[problem], its cost and state trajectory are stored.  Initialise
 * best_cost to a large FINITE value (3e38; the library is built with -ffinite-math-only); it carries over between calls
 * like the reference's attribute.
 * How the work is laid out (T <= 64: mean + scale_tril @ eps of all samples on the matrix pipe; 8 or 16 waves per
 * problem depending on NP) does not show in the results: a problem's outputs are the same bits whatever NP is.
 * ------------------------------------------------------------------------------------------- */
int mpb_mppi_step(float *mean, const float *eps, const float *scale_tril, const float *cov_inv,
                  const float *state0, const float *goal, const float *ctrl_min, const float *ctrl_max,
                  const float *discount, const float *c_weights, const float *geom, int geom_flags,
                  float *controls, float *states, float *costs, float *weights,
                  float *best_cost, float *best_states,
                  int NP, int S, int T, int c, int control_type, float dt,
                  float k_sigma, float weight, float temp, float step_size,
                  int n_iters, uint64_t seed, uint32_t iter0, void *stream);
/* How mpb_mppi_step would launch a shape, without launching anything (the same function decides both; the MPB_MPPI_WAVES /
 * MPB_MPPI_NOISE / MPB_MPPI_NO_GRID tuning variables, read once per process, are part of it).  geom_flags, NP, S, T, c as for
 * mpb_mppi_step; has_geom / has_eps: whether its geom / eps would be non-NULL (eps picks the kernel instantiation only: the plan
 * does not depend on it); n_cu: the compute units to plan for, <= 0 asks the current device.  plan[0..3] receive
 *   [0] the noise product: MPB_MPPI_NOISE_GLOBAL (per lane, factor in global memory), _LDS (per lane, transposed factor in LDS),
 *       _MATRIX (all samples on the matrix pipe, T <= 64);
 *   [1] waves per problem;  [2] cells of the broad-phase grid staged in LDS (0: the exhaustive collision walk);
 *   [3] dynamic LDS of the launch in bytes.
 * Returns what mpb_mppi_step would return for the shape (MPB_E_INVALID: bad shape, MPB_E_UNSUPPORTED: the controls slab does not
 * fit LDS; plan[] is zero then). */
#define MPB_MPPI_NOISE_GLOBAL 0
#define MPB_MPPI_NOISE_LDS 1
#define MPB_MPPI_NOISE_MATRIX 2
int mpb_mppi_plan(int geom_flags, int has_geom, int NP, int S, int T, int c, int has_eps, int n_cu, int *plan);
/* The point-particle system as stand-alone entry points, for code written against the reference's system object
 * (dynamics/point.py); mpb_mppi_step fuses the same arithmetic.
 * mpb_point_dynamics -- PointParticleDynamics.dynamics (point.py:102-140): x_next = x + (clamp(u, ctrl_min, ctrl_max) +
 *   dyn_std * noise) * dt over n rows of `dim` entries (the reference's xdot = cat(x[..., state_dim:], u) has an empty
 *   first part); noise NULL = deterministic, else (n, dim) standard normals (the reference draws them with torch.randn).
 * mpb_point_traj_cost -- PointParticleDynamics.traj_cost (point.py:154-226): X (T, B, state_dim), U (T, B, ctrl_dim) in the
 *   reference's time-major layout, goal (state_dim), discount (T) -> costs (B) = sum_t disc_t (w_pos |X - goal|^2 +
 *   w_ctrl |U|^2) + w_pos_T disc_{T-1} |X_{T-1} - goal|^2 + energy; w_vel is accepted and unused (quirk Q8: the reference
 *   slices dX[..., state_dim:control_dim], an empty tensor); `energy` is the scalar the caller's cost object contributes
 *   (quirk Q6: cost.eval(cat(X, U)).sum(-1) collapses to ONE number added to every rollout; 0 without one). */
int mpb_point_dynamics(const float *x, const float *u, const float *ctrl_min, const float *ctrl_max, const float *dyn_std,
                       const float *noise, float *x_next, size_t n, int dim, float dt, void *stream);
int mpb_point_traj_cost(const float *X, const float *U, const float *goal, const float *discount, float w_pos, float w_vel,
                        float w_ctrl, float w_pos_T, float energy, float *costs, int T, int B, int state_dim, int ctrl_dim,
                        void *stream);


/* ---------------------------------------------------------------------------------------------
 * StochGPMP -- replaces StochGPMP.sample_and_eval / _get_costs / _update_distribution
 * (stoch_gpmp.py:235-279).  One iteration is three calls:
 *   mpb_gp_prior_sample   samples (P*S,H,2D) around the particle means from the sampling prior (below);
 *   mpb_stoch_gpmp_costs  costs (P,S) = CostGP.eval + CostGoalPrior.eval + CostCollision.eval
 *                         (cost_functions.py:271-289, :520-536, :171-189) + T * V Sigma^-1 U^T
 *                         (stoch_gpmp.py:239-241), evaluated factor-wise without the dense Sigma^-1;
 *                         means (P,H,2D) particle means, start / goal (P,2D);
 *   mpb_stomp_update      with Sigma == NULL: softmax over S and means += lr * sum_s w_s (sample_s - mean)
 *                         (stoch_gpmp.py:267-275, no covariance in the update).
 * ------------------------------------------------------------------------------------------- */
int mpb_stoch_gpmp_costs(const float *samples, const float *means, const float *start, const float *goal,
                         const float *geom, float *costs, int P, int S, int H, int D, float dt,
                         float sigma_start, float sigma_gp, float sigma_goal, float sigma_coll,
                         float sigma_start_sample, float sigma_gp_sample, float sigma_goal_sample,
                         float temperature, void *stream);

/* The whole loop, n_iters iterations enqueued by one call (device Philox noise, iteration i draws with seed + i exactly
 * like n_iters single-iteration rounds of the three calls above): means (P,H,2D) in/out; means64 (P,H,2D) fp64 scratch;
 * samples (P*S,H,2D), costs (P,S), weights (P,S): outputs of the last iteration; Udiag / Uoff / scale_tril: the sampling
 * prior as for mpb_gp_prior_sample(_dense) (scale_tril NULL or H > 128: chain form).  The whole envelope of the three stages
 * (3 <= H <= MPB_MAX_H, 1 <= D <= MPB_MAX_DOF, mpb_stomp_update's LDS budget) is checked before anything is enqueued;
 * mpb_stoch_gpmp_costs alone also takes H = 2. */
int mpb_stoch_gpmp_step(float *means, double *means64, float *samples, float *costs, float *weights,
                        const double *Udiag, const double *Uoff, const double *scale_tril,
                        const float *start, const float *goal, const float *geom,
                        int P, int S, int H, int D, float dt,
                        float sigma_start, float sigma_gp, float sigma_goal, float sigma_coll,
                        float sigma_start_sample, float sigma_gp_sample, float sigma_goal_sample,
                        float temperature, float step_size, int n_iters, uint64_t seed, void *stream);

/* ---------------------------------------------------------------------------------------------
 * GP-prior initial particles -- replaces OptimizationPlanner.get_random_trajs (base.py:155-202) over
 * MultiMPPrior (costs/factors/mp_priors_multi.py:100-110, :213-256): x = mean + scale_tril @ eps with
 * scale_tril = U^-T, K^-1 = U U^T block upper-bidiagonal with (2x2) (x) I_D blocks (fp64 throughout).
 * out (G*n, H, 2D) fp32, particle index = mode * n + sample (base.py:202); means (G,H,2D) fp64;
 * eps NULL -> device Philox, else (n, G, H*2D) fp64 standard normals (MultivariateNormal draw order);
 * Udiag (H,3) = (u00,u01,u11) of U_tt, Uoff (H-1,4) = row-major 2x2 U_{t,t+1}; both fp64, device.
 * ------------------------------------------------------------------------------------------- */
int mpb_gp_prior_sample(float *out, const double *means, const double *eps, const double *Udiag,
                        const double *Uoff, int G, int n, int H, int D, uint64_t seed, void *stream);
/* Same samples from the dense per-dof scale_tril (2H x 2H row-major fp64, index 2t + {0: position, 1: velocity};
 * = U_dof^-T, what MultivariateNormal(precision_matrix=...) holds for one degree of freedom) as a GEMM on the
 * matrix cores (v_mfma_f64_16x16x4_f64); H <= 128.  Same Philox stream as mpb_gp_prior_sample. */
int mpb_gp_prior_sample_dense(float *out, const double *means, const double *eps, const double *scale_tril,
                              int G, int n, int H, int D, uint64_t seed, void *stream);
/* MultiMPPrior with ARBITRARY start / GP / goal precisions (mp_priors_multi.py:213-256 accepts any matrices; the planners
 * of the reference pass isotropic ones, which the two entries above serve): x = mean + L eps from the dense M x M
 * scale_tril L of the whole trajectory (M = 2D*H <= 4096), handed over TRANSPOSED (tril_t[k*M + m] = L[m][k], fp64).
 * means (G,M) fp64; eps NULL (device Philox) or (n,G,M) fp64; out (G*n, M) fp32, index mode * n + sample. */
int mpb_mvn_sample_dense(float *out, const double *means, const double *eps, const double *tril_t,
                         int G, int n, int M, uint64_t seed, void *stream);

/* ---------------------------------------------------------------------------------------------
 * torch's CPU generator on the device (noise = 'mt19937'): n_calls successive `torch.empty(n).normal_()` draws of a
 * contiguous fp32 block of n >= 16 elements from torch's mt19937 state, written to out (n_calls, n) -- the uniforms and the
 * state bit for bit, the normals within a few ULP (torch's vectorised log / sincos are not restated).  Host side and tables:
 * motion_planning_baselines_amd/mt19937.py; kernels: csrc/mpb_mt19937.h.  Three launches: a prefix of 20 560 raw words from
 * state_in (one workgroup), the first 624 words of every segment by jump ahead (one workgroup per segment, the prefix in 83 KB
 * of LDS), and the segments' words, tempered and Box-Muller'd (one workgroup per segment).
 * state_in: torch's 624-word array (device, uint32); pos: the index of the next word drawn, 624 when `left` == 1, else `next`;
 * state_out (may alias state_in): torch's array after the draw, the 624 words at final_idx of the final window (-1: the draw
 * does not reach the end of the array, which is copied); segs (n_segs, 4) int: call, first 16-chunk, 16-chunks, last segment
 * of its call; jump_idx (n_segs + 1, jump_stride) uint16, jump_cnt (n_segs + 1): the set coefficients of t^offset mod phi
 * per segment and for the final window, padded to a multiple of 8 with 20 560; work: 20 608 + 624 (n_segs + 1) words of
 * scratch that every call writes (one per stream).  The same draw with events around its launches: mpb_debug.h.
 * Measured at C3 (16 calls of 3 670 016, 256 segments): prefix 0.026 ms, jump 0.21 ms, generation 0.31 ms a draw.
 * ------------------------------------------------------------------------------------------- */
int mpb_mt19937_normals(float *out, int n, int n_calls, const uint32_t *state_in, int pos, int final_idx, uint32_t *state_out,
                        const uint16_t *jump_idx, const int *jump_cnt, int jump_stride, const int *segs, int n_segs,
                        uint32_t *work, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Collision predicate (build-defined; the reference asks torch_robotics' task.compute_collision, rrt_base.py:100-101):
 * a configuration is in collision iff the per-waypoint collision cost above is positive,
 *   gap = sum_f s_f sum_l relu(margin + r_l - min_o sdf_o(x_l(q))) > 0.
 * q (N,D); in_collision (N) bytes, 0 / 1; gap (N) optional (may be NULL): the hinge sum.  geom_flags as above.
 * ------------------------------------------------------------------------------------------- */
int mpb_collision_check(const float *q, const float *geom, int geom_flags, unsigned char *in_collision, float *gap,
                        int N, int D, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Validation of a batch of trajectories (build-defined; the reference's examples ask torch_robotics'
 * task.get_trajs_collision_and_free / compute_fraction_free_trajs / compute_collision_intensity_trajs /
 * compute_success_free_trajs, panda_spheres_CHOMP.py:126, :146-148): one launch, one workgroup per trajectory, no dense
 * point is ever stored.
 * trajs: N trajectories of H rows, read in place; row h of trajectory n starts at trajs + (n*H + h)*row_stride and its first
 *   D floats are the joint positions (row_stride >= D; the columns D .. row_stride-1 -- the velocity half of a state
 *   trajectory, or anything else -- are never read).
 * Dense points: P = (H-1)(n_interp+1) + 1 per trajectory, the points of mpb_traj_interpolate above: point
 *   p = seg*(n_interp+1) + k is x0 + ((float)k / (float)(n_interp+1)) * (x1 - x0), the waypoint's own bits for k = 0 and for
 *   the last point.  A dense point is in collision iff mpb_collision_check says so of it (gap > 0, margin included).
 * n_in_collision (N): dense points in collision; first_in_collision (N): the smallest such p, -1 when there is none;
 * max_gap (N): the largest hinge sum (mpb_collision_check's gap) over the dense points, 0 when the trajectory is free;
 * point_in_collision (N, P) bytes, 0 / 1: optional (may be NULL).  No atomics: the same bits on every run.
 * Refusals, in this order: D > MPB_MAX_DOF: MPB_E_UNSUPPORTED; N < 0, H < 2, D < 1, n_interp < 0, row_stride < D or P beyond
 * an int: MPB_E_INVALID; (N == 0: MPB_OK, nothing launched;) a null required pointer, geom not 16-byte aligned: MPB_E_INVALID.
 * ------------------------------------------------------------------------------------------- */
int mpb_traj_collision_stats(const float *trajs, size_t row_stride, const float *geom, int geom_flags, int n_interp,
                             int *n_in_collision, int *first_in_collision, float *max_gap, unsigned char *point_in_collision,
                             int N, int H, int D, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Self-collision field: the robot's collision spheres against each other (build-defined; the reference's Panda
 * examples get this field from torch_robotics with use_self_collision_storm=True).  Serial chains only.
 *   c(q) = sum over pairs (a, b) of relu(T_ab - |x_a(q) - x_b(q)|),   T_ab = margin + r_a + r_b,
 * x_l the collision-sphere centres mpb_fk_collision_points gives; a configuration collides with itself iff c(q) > 0 (the rule of
 * mpb_collision_check).  Gradient of an active pair (T_ab - n > 0, n = |x_a - x_b|): d c / d x_a = -(x_a - x_b) / n,
 * d c / d x_b = +(x_a - x_b) / n, d c / d q = J^T of that; a pair with n == 0 contributes zero.
 *
 * The self buffer is ONE self-contained array of 32-bit words with a magic and version of its own (mpb_self_layout.h, generated
 * from self_layout.py -- the one definition): a header of MPB_SELF_HEADER_WORDS words (MPB_SW_MAGIC, _VERSION, _N_DOF, _N_TF =
 * n_dof + 1, _N_LINKS, _N_PAIRS, _MARGIN, the section offsets _OFF_TF, _OFF_LINKS, _OFF_PAIRS, _TOTAL; the rest zero), then the
 * joint transforms (n_tf x 12) and the link table (n_links x 8) in the row formats of the geometry buffer -- EVERY link, the pair
 * indices are positions in this table --, then the pair table, MPB_SELF_PAIR_WORDS words per pair: a | b << MPB_SELF_PAIR_B_SHIFT
 * with a < b < n_links, and T_ab as fp32.  Limits: MPB_SELF_MAX_LINKS spheres, MPB_SELF_MAX_PAIRS pairs.
 *
 * mpb_self_check validates such a buffer held in HOST memory (n_words must equal its total): header, offsets, limits, link
 * frames sorted in [1, n_dof + 1], every pair a < b < n_links with a positive finite threshold.
 *
 * The three device entry points take the buffer in DEVICE memory, 16-byte aligned.  The caller validates it with
 * mpb_self_check before uploading it: the entry points have no host copy.  They read its 16 header words back ONCE per buffer
 * address and device (a synchronous 64-byte copy on the first call with that pointer: make that call outside stream capture),
 * check the header alone and size the launch's LDS from n_links: 768 bytes per sphere, twice that with gradients.  The kernels
 * compare the header (magic, n_dof, n_links, n_pairs) with the numbers they were launched with and answer NaN (in_collision = 1) when it has changed since.
 * mpb_self_invalidate(self) forgets what was read at that address: call it whenever ANOTHER self buffer is written to device memory
 * at an address an earlier call may have seen (an allocator hands a freed block out again).  Host only, never fails.
 *
 * mpb_self_collision_eval:  out[b] (+)= weight * k_sigma * sum_{h >= h_begin} c(trajs[b, h, :n_dof]);  trajs (B, H, d), d >= n_dof;
 *   per_waypoint (B, H) optional (may be NULL): c un-scaled, 0 for h < h_begin.
 * mpb_self_collision_grad:  the same out, and grad (B, H, d) (+)= d out[b] / d trajs[b]; when not accumulating the velocity
 *   channels n_dof .. d-1 are written 0, when accumulating they are left alone.
 *   accumulate != 0 adds onto out AND grad (CHOMP adds the self gradient onto the obstacle gradient): the old value plus the
 *   fresh one in ONE fp32 rounding, so accumulating equals the buffer plus a fresh evaluation bit for bit.
 * mpb_self_collision_check: q (N, D) with D == n_dof; in_collision (N) bytes 0 / 1 = c > 0; gap (N) optional: c.  or_into != 0 ORs
 *   into the existing flags and adds c onto the existing gap (after mpb_collision_check: collides with the world OR with itself).
 * One wave per trajectory, one lane per waypoint (check: one lane per configuration).  Sums in fixed order (pairs in table order
 * in fp32, then a fixed wave reduction): the same bits on every run.
 * Refusals, in this order: rows wider than positions + velocities of MPB_MAX_DOF joints (d > 2 MPB_MAX_DOF; check: D >
 * MPB_MAX_DOF): MPB_E_UNSUPPORTED; B < 0, H < 1, d < 1, h_begin < 0 (check: N < 0, D < 1): MPB_E_INVALID; (B == 0 / N == 0:
 * MPB_OK, nothing launched;) a null required pointer, a self buffer not 16-byte aligned: MPB_E_INVALID; the header: bad magic /
 * version / offsets: MPB_E_INVALID, n_dof > MPB_MAX_DOF, n_links > MPB_SELF_MAX_LINKS, n_pairs > MPB_SELF_MAX_PAIRS:
 * MPB_E_UNSUPPORTED, d < n_dof (check: D != n_dof): MPB_E_INVALID.
 * ------------------------------------------------------------------------------------------- */
int mpb_self_check(const float *self_host, int n_words);
int mpb_self_invalidate(const float *self);
int mpb_self_collision_eval(const float *trajs, const float *self, float *out, float *per_waypoint,
                            int B, int H, int d, int h_begin, float k_sigma, float weight, int accumulate, void *stream);
int mpb_self_collision_grad(const float *trajs, const float *self, float *out, float *grad,
                            int B, int H, int d, int h_begin, float k_sigma, float weight, int accumulate, void *stream);
int mpb_self_collision_check(const float *q, const float *self, unsigned char *in_collision, float *gap,
                             int N, int D, int or_into, void *stream);

/* ---------------------------------------------------------------------------------------------
 * SDF-grid field: a precomputed lattice of signed distances, interpolated at the robot's collision spheres (build-defined, DESIGN.md
 * 10; the reference's examples build their environments with precompute_sdf_obj_fixed=True, sdf_cell_size=...).  Serves arbitrary
 * geometry (the caller supplies the node values) at a cost that does not depend on what the scene holds.
 *   grid:  (nx, ny, nz) fp32 nodes, node (i, j, k) at lo + (i, j, k) * cell (one cell for all axes), word (k * ny + j) * nx + i of
 *          the node section; nz == 1: planar, z ignored, bilinear.  Limits: every dimension in 2..MPB_SDF_MAX_DIM (nz: or 1),
 *          at most MPB_SDF_MAX_NODES nodes; 32-bit index arithmetic throughout.
 *   s(x):  per axis u = (x - lo) * inv_cell (inv_cell = fl32(1 / cell), a header word), clamped to [0, n - 1]; i0 = min(floor(u),
 *          n - 2); f = u - i0; lerp form fmaf(f, v1 - v0, v0) along x, then y, then z -- a point with f == 0 on every axis returns
 *          that node's bits.  A point outside the box takes the value of the nearest boundary point and gradient 0 along every axis
 *          it lies outside on: the grid is expected to cover the workspace.
 *   c(q) = sum_l relu(margin + r_l - s(x_l(q)))  over the robot's collision spheres (x_l: mpb_fk_collision_points; a point robot has
 *          its one sphere at q, z = 0 with two coordinates); in collision iff c(q) > 0 (the rule of mpb_collision_check).
 *   gradient: an active sphere (margin + r_l - s > 0) contributes -grad s(x_l) through J^T, grad s the exact derivative of the
 *          interpolant (piecewise constant along its own axis), from the same eight (planar: four) node loads as the value.
 *
 * The SDF buffer is ONE self-contained array of 32-bit words with a magic and version of its own (mpb_sdf_layout.h, generated from
 * sdf_layout.py -- the one definition): a header of MPB_SDF_HEADER_WORDS words (MPB_DW_MAGIC, _VERSION, _KIND = MPB_KIND_POINT /
 * _CHAIN, _N_DOF, _N_TF = n_dof + 1 or 0 for a point robot, _N_LINKS, _MARGIN, _DIMS (3), _LO (3), _CELL, _INV_CELL, the section
 * offsets _OFF_TF, _OFF_LINKS, _OFF_NODES (a multiple of MPB_SDF_NODE_ALIGN words), _TOTAL; the rest zero), then the joint transforms
 * (n_tf x 12) and the link table (n_links x 8) in the row formats of the geometry buffer, EVERY link, then the nodes.
 *
 * mpb_sdf_grid_check validates such a buffer held in HOST memory (n_words must equal its total): magic / version, kind, limits
 * (n_dof, n_links, dimensions, node count), the transforms a kind needs, a planar grid only with a point robot, offsets and total,
 * cell positive and finite with inv_cell its fp32 reciprocal, margin and lo finite, link frames sorted in [1, n_dof + 1].  It reads
 * the words before the node section alone: the node values are the caller's to check (geometry.GridSDFField refuses non-finite
 * ones), and a caller whose nodes are built on the device may pass those leading words with the whole buffer's n_words.
 *
 * The device entry points take the buffer in DEVICE memory, 16-byte aligned, validated by the caller before the upload.  They read
 * its 32 header words back ONCE per buffer address and device (a synchronous 128-byte copy on the first call with that pointer:
 * make that call outside stream capture) and check the header alone.  The kernels form every node index from the dimensions they
 * were launched with, clamped into the grid whatever the input, compare the header (magic, n_dof, n_links, dims) with those numbers
 * and answer NaN (in_collision = 1; the builder: nothing written) when it has changed since.  mpb_sdf_grid_invalidate(sdf) forgets
 * what was read at that address: call it whenever ANOTHER SDF buffer is written at an address an earlier call may have seen.
 *
 * mpb_sdf_grid_build: fills the node section of `sdf` with min_o sd_o(node position) over the spheres and boxes of ONE packed
 *   CollisionField `geom` (a geometry buffer in device memory, any robot; a chain of fields is refused), node position
 *   fmaf(i, cell, lo) per axis, the signed distances every cost kernel takes.  One thread per node.  Reads both headers back
 *   synchronously.  Refusals in this order: null pointer, alignment, the SDF header, the geometry header (magic / version: INVALID;
 *   chained: UNSUPPORTED; no obstacle: INVALID).
 * mpb_sdf_grid_build_occupancy: fills the node section of `sdf` from an occupancy voxel map (a scan): `occupancy` is nx * ny * nz bytes
 *   in node order in device memory, read only; a node is the centre of a voxel of edge `cell`, a byte != 0 says that voxel is solid, the
 *   surface is the set of voxel faces between a solid and a free voxel.  Integer part, exact: D2 of a free node = the smallest squared
 *   index distance di^2 + dj^2 + dk^2 to an occupied node, D2 of an occupied node = the smallest to a free node, and D2 = D2_none =
 *   (nx-1)^2 + (ny-1)^2 + (nz-1)^2 + 1 when the other class has no member (D2 < 2^24: exact in fp32).  Float part, bit-defined: node
 *   value v = cell * (sqrt(D2) - 0.5) for a free node, -v for an occupied one, in fp32 as three separately rounded operations (a
 *   correctly rounded root, a subtract, a multiply; no fma), `cell` the header's fp32 word.  Against an exact field whose obstacles lie
 *   inside the grid and are unions of balls of radius >= (sqrt(3)/2) cell: free nodes -(sqrt(3) - 1/2) cell <= sdf - v < cell / 2,
 *   occupied nodes sdf - v > -cell / 2.  A separable transform, one pass per axis (x, y, then z; a planar grid has no z pass), in
 *   place: the partial squared distances live in the node section as int32 until the last pass writes fp32; no workspace, no atomics,
 *   the same bits on every run.  Dimensions from the cached header read, as for the other device entry points.  Refusals in this
 *   order: null pointer, alignment of `sdf`, the SDF header.
 * mpb_sdf_grid_sample: points (N, 3) -> s (N) and, when grad is not NULL, grad (N, 3) = d s / d x.  No robot.  Refusals: N < 0:
 *   INVALID; (N == 0: MPB_OK, nothing launched;) null pointer; alignment; the header.
 * mpb_sdf_grid_eval / _grad: the signature and meaning of mpb_self_collision_eval / _grad, c as above: out[b] (+)= weight * k_sigma *
 *   sum_{h >= h_begin} c(trajs[b, h, :n_dof]); per_waypoint (B, H) optional: c un-scaled, 0 for h < h_begin; grad (B, H, d) (+)=
 *   d out[b] / d trajs[b], the velocity channels n_dof .. d-1 written 0 when not accumulating and left alone when accumulating;
 *   accumulate != 0 adds the fresh value in ONE fp32 rounding.  One wave per trajectory, one lane per waypoint, trips of 64; sums in
 *   fixed order: the same bits on every run.
 * mpb_sdf_grid_collision_check: q (N, D) with D == n_dof; in_collision (N) bytes 0 / 1 = c > 0; gap (N) optional: c; or_into != 0
 *   ORs into the existing flags and adds c onto the existing gap -- the signature and meaning of mpb_self_collision_check.
 * Refusals of the last three, in this order: d > 2 MPB_MAX_DOF (check: D > MPB_MAX_DOF): MPB_E_UNSUPPORTED; B < 0, H < 1, d < 1,
 * h_begin < 0 (check: N < 0, D < 1): MPB_E_INVALID; (B == 0 / N == 0: MPB_OK, nothing launched;) a null required pointer, an SDF
 * buffer not 16-byte aligned: MPB_E_INVALID; the header: as mpb_sdf_grid_check says; d < n_dof (check: D != n_dof): MPB_E_INVALID.
 * ------------------------------------------------------------------------------------------- */
int mpb_sdf_grid_check(const float *sdf_host, int n_words);
int mpb_sdf_grid_invalidate(const float *sdf);
int mpb_sdf_grid_build(const float *geom, float *sdf, void *stream);
int mpb_sdf_grid_build_occupancy(const unsigned char *occupancy, float *sdf, void *stream);
int mpb_sdf_grid_sample(const float *points, const float *sdf, float *s, float *grad, int N, void *stream);
int mpb_sdf_grid_eval(const float *trajs, const float *sdf, float *out, float *per_waypoint,
                      int B, int H, int d, int h_begin, float k_sigma, float weight, int accumulate, void *stream);
int mpb_sdf_grid_grad(const float *trajs, const float *sdf, float *out, float *grad,
                      int B, int H, int d, int h_begin, float k_sigma, float weight, int accumulate, void *stream);
int mpb_sdf_grid_collision_check(const float *q, const float *sdf, unsigned char *in_collision, float *gap,
                                 int N, int D, int or_into, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Moving-obstacle field: spheres and axis-aligned boxes whose centres depend on the ROW of the trajectory (build-defined, DESIGN.md
 * 10).  Row h sees the world at one time t_h; the host has evaluated every centre c_{o,h} for every row (geometry.MovingObstacleField:
 * piecewise linear between keyframes, in fp64, rounded once).  Boxes translate and do not rotate.
 *   c_h(q) = sum_l relu(margin + r_l - min_o sd_{o,h}(x_l(q)))   over the robot's collision spheres (x_l: mpb_fk_collision_points; a
 *          point robot has its one sphere at q, z = 0 with two coordinates); sd of a sphere |x - c_{o,h}| - R_o, of a box the
 *          expression every cost kernel takes with centre c_{o,h}; spheres in table order, then boxes, a strict < keeps the first
 *          minimum.  Row h is in collision iff c_h(q_h) > 0.
 *   gradient: an active sphere contributes -grad sd of its nearest obstacle through J^T, with the conventions of the static field
 *          (|x - c|^2 clamped at 1e-30; inside a box the unit axis of the largest component, the first on ties).  Time is fixed per
 *          row: the obstacles' velocity is no part of d c / d q.
 *
 * The moving-obstacle buffer is ONE self-contained array of 32-bit words with a magic and version of its own (mpb_moving_layout.h,
 * generated from moving_layout.py -- the one definition): a header of MPB_MOVING_HEADER_WORDS words (MPB_VW_MAGIC, _VERSION, _N_DOF,
 * _N_TF = n_dof + 1 or 0 for a point robot, _N_LINKS, _N_ROWS, _N_SPHERES, _N_BOXES, _MARGIN, the section offsets _OFF_TF, _OFF_LINKS,
 * _OFF_RADII, _OFF_HALF, _OFF_CENTRES, _TOTAL; the rest zero), then -- each at a multiple of MPB_MOVING_ALIGN words -- the joint
 * transforms (n_tf x 12) and the link table (n_links x 8) in the row formats of the geometry buffer, EVERY link; the sphere radii
 * (n_spheres, zero-padded to a multiple of MPB_MOVING_ALIGN); the box half extents (n_boxes x 4: hx, hy, hz, 0); the centres as
 * [obstacle][x|y|z][row], spheres first, the row axis padded to a multiple of MPB_MOVING_ROW_PAD by repeating row n_rows - 1 (the
 * lanes of a trip read 64 consecutive words and never past the table).  Limits: MPB_MOVING_MAX_ROWS rows, MPB_MOVING_MAX_SPHERES
 * spheres, MPB_MOVING_MAX_BOXES boxes (at least one obstacle), MPB_MOVING_MAX_LINKS collision spheres of the robot.
 *
 * mpb_moving_check validates such a buffer held in HOST memory (n_words must equal its total): magic / version, limits, the transforms
 * a robot kind needs, offsets and total, a finite margin, link frames sorted in [1, n_dof + 1], positive finite radii and half
 * extents, finite centres, padding rows that repeat the last row.
 *
 * The device entry points take the buffer in DEVICE memory, 16-byte aligned, validated by the caller before the upload.  They read
 * its 16 header words back ONCE per buffer address and device (a synchronous 64-byte copy on the first call with that pointer: make
 * that call outside stream capture) and check the header alone.  H must equal the buffer's n_rows -- the centres were evaluated for
 * exactly those rows --: otherwise MPB_E_INVALID, and mpb_last_error names both numbers.  The kernels form every centre index from
 * the numbers they were launched with, compare the header (magic, n_dof, n_links, n_rows, n_spheres, n_boxes) with them and answer NaN
 * (in_collision = 1) when it has changed since.  mpb_moving_invalidate(moving) forgets what was read at that address: call it whenever
 * ANOTHER buffer is written at an address an earlier call may have seen.  Host only, never fails.
 *
 * mpb_moving_collision_eval / _grad: the signature and meaning of mpb_self_collision_eval / _grad with c_h as above: out[b] (+)= weight
 *   * k_sigma * sum_{h >= h_begin} c_h(trajs[b, h, :n_dof]); per_waypoint (B, H) optional: c_h un-scaled, 0 for h < h_begin; grad
 *   (B, H, d) (+)= d out[b] / d trajs[b], the velocity channels n_dof .. d-1 written 0 when not accumulating and left alone when
 *   accumulating; accumulate != 0 adds the fresh value in ONE fp32 rounding.
 * mpb_moving_collision_check: per ROW, because the predicate needs the row's time: trajs (B, H, d), d >= n_dof; in_collision (B * H)
 *   bytes 0 / 1 = c_h > 0; gap (B * H) optional: c_h; or_into != 0 ORs into the existing flags and adds c_h onto the existing gap.
 * One wave per trajectory, one lane per row, trips of 64; no LDS, no atomics; sums in fixed order (spheres in table order in fp32,
 * a lane's rows ascending, a fixed wave reduction): the same bits on every run.
 * Refusals, in this order: d > 2 MPB_MAX_DOF: MPB_E_UNSUPPORTED; B < 0, H < 1, d < 1, h_begin < 0: MPB_E_INVALID; (B == 0: MPB_OK,
 * nothing launched;) a null required pointer, a buffer not 16-byte aligned: MPB_E_INVALID; the header: as mpb_moving_check says of
 * it; d < n_dof: MPB_E_INVALID; H != n_rows: MPB_E_INVALID.
 * ------------------------------------------------------------------------------------------- */
int mpb_moving_check(const float *moving_host, int n_words);
int mpb_moving_invalidate(const float *moving);
int mpb_moving_collision_eval(const float *trajs, const float *moving, float *out, float *per_waypoint,
                              int B, int H, int d, int h_begin, float k_sigma, float weight, int accumulate, void *stream);
int mpb_moving_collision_grad(const float *trajs, const float *moving, float *out, float *grad,
                              int B, int H, int d, int h_begin, float k_sigma, float weight, int accumulate, void *stream);
int mpb_moving_collision_check(const float *trajs, const float *moving, unsigned char *in_collision, float *gap,
                               int B, int H, int d, int or_into, void *stream);

/* ---------------------------------------------------------------------------------------------
 * SDF grid from triangle meshes: the exact signed distance to a mesh at every node (build-defined).
 *   mesh:  triangles (a, b, c), counter-clockwise seen from outside, as ONE self-contained array of 32-bit words with a magic and
 *          version of its own (mpb_mesh_layout.h, generated from mesh_layout.py -- the one definition): a header of
 *          MPB_MESH_HEADER_WORDS words (MPB_MW_MAGIC, _VERSION, _N_TRI in 1..MPB_MESH_MAX_TRIS, _N_GROUPS = ceil(n_tri / MPB_MESH_GROUP),
 *          _SIGNED 0 / 1, _THICKNESS >= 0, _BB_LO (3), _BB_HI (3), _OFF_TRIS = MPB_MESH_HEADER_WORDS, _OFF_BOXES, _TOTAL; the rest zero);
 *          n_groups * MPB_MESH_GROUP triangle records of MPB_MESH_TRI_WORDS words -- MPB_TRI_A, _B, _C, the unit face normal _N_FACE,
 *          the pseudonormals of the edges _N_AB, _N_BC, _N_CA (sum of the two faces' unit normals) and of the vertices _N_A, _N_B, _N_C
 *          (angle-weighted sum of the faces' normals), two zero words; the records beyond n_tri repeat record n_tri - 1 --; then one box
 *          of MPB_MESH_BOX_WORDS words per group of MPB_MESH_GROUP consecutive records: lo (3), 0, hi (3), 0, containing the group's
 *          fp32 vertices.  The pseudonormals are computed in fp64 and rounded to fp32 once per edge / vertex: every record that shares
 *          an edge or a vertex carries the same bits.
 *   node:  p = fmaf(i, cell, lo) per axis, as mpb_sdf_grid_build forms it.  With a pose [R | t] (mesh frame to grid frame, row-major
 *          3 x 4) the node is taken into the mesh frame, p' = R^T (p - t):  d = p - t per axis (one rounding each), then per axis m
 *          p'_m = fmaf(R[2][m], d_z, fmaf(R[1][m], d_y, R[0][m] * d_x)).  A null pose leaves p untouched, bit for bit.
 *   distance to one triangle, in fp32 with contraction off, every dot product dot(u, v) = fmaf(u_z, v_z, fmaf(u_y, v_y, u_x * v_x)):
 *          ab = b - a, ac = c - a, bc = c - b, ap = p - a, bp = p - b, cp = p - c; d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp),
 *          d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp); vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4
 *          (two rounded products, one rounded difference).  The region walk of Ericson, Real-Time Collision Detection 5.1.5, vertex
 *          regions first, then edge regions, then the face -- the first that holds names the feature:
 *            A:  d1 <= 0 and d2 <= 0;   B:  d3 >= 0 and d4 <= d3;   C:  d6 >= 0 and d5 <= d6;
 *            AB: vc <= 0, d1 >= 0, d3 <= 0, u = d1 / (d1 - d3) along ab from a;
 *            CA: vb <= 0, d2 >= 0, d6 <= 0, u = d2 / (d2 - d6) along ac from a;
 *            BC: va <= 0, d4 - d3 >= 0, d5 - d6 >= 0, u = (d4 - d3) / ((d4 - d3) + (d5 - d6)) along bc from b;
 *            face: u = vb / (va + vb + vc) along ab, w = vc / (va + vb + vc) along ac, from a.
 *          A quotient n / m is n * (1.0f / m), the reciprocal a correctly rounded division; u is clamped to [0, 1], w to [0, 1 - u]: the
 *          point c = base + u e1 + w e2 lies on the triangle whatever the rounding.  The offset is taken from the base's difference,
 *          r = fmaf(-w, e2, fmaf(-u, e1, p - base)) per axis, and dist2 = dot(r, r).
 *   winner: the triangle with the smallest dist2; triangles are visited in ascending record order and a candidate replaces the best
 *          only when strictly smaller: the winner is unique, a padding record never wins.
 *   sign:  s = dot(r, n_feature) of the winner (Baerentzen and Aanaes: the angle-weighted pseudonormal); s < 0 is inside.
 *   value: a signed mesh v = sqrt(dist2) outside, -sqrt(dist2) inside; an unsigned mesh (open surfaces, scans) v = sqrt(dist2) -
 *          thickness; the root correctly rounded.
 *
 * mpb_mesh_check validates a mesh buffer held in HOST memory (n_words must equal its total): magic / version, counts within limits,
 * signed 0 / 1, thickness finite and >= 0, offsets and total, every float word finite, every record inside its group's box, every
 * box inside the header's.
 *
 * mpb_sdf_grid_build_mesh: fills the node section of `sdf` with v.  `mesh` and `sdf` in device memory, 16-byte aligned; `pose_host`
 *   12 floats in HOST memory, read during the call, or NULL.  The grid's dimensions, lo and cell come from the cached SDF header read,
 *   as for the other builders; the mesh header is read back the same way (once per address and device) and compared in the kernel:
 *   when either has changed, nothing is written.  mpb_sdf_grid_invalidate(mesh) forgets a mesh buffer's address too.
 *   flags: MPB_MESH_MIN: the node becomes min(what it holds, v) -- several meshes, each with a pose of its own, or a mesh on top of
 *   an mpb_sdf_grid_build, give the union; MPB_MESH_NO_CULL: every group is visited.  Otherwise groups are culled, exactly: pass 1 gives
 *   each node the smallest, over groups, squared distance to the box's farthest corner (an upper bound of its dist2); in pass 2 a group
 *   is skipped for a wave (a block of 4 x 4 x 4 nodes, planar 8 x 8) when no lane's squared distance to the box is at or below
 *   min(best so far, pass-1 bound) + slack, slack = 2^-14 M^2 with M the largest absolute coordinate among the nodes (in the mesh
 *   frame) and the mesh's box (DESIGN.md 10 derives it).  The bound only culls: the same triangle wins with and without culling, the
 *   node bits are identical.  One thread per node, triangle records through uniform loads, no LDS, no atomics, no cross-lane
 *   arithmetic: the same bits on every run.  Refusals in this order: null pointer, alignment, the SDF header, the mesh header,
 *   unknown flag bits, a pose that is not finite: MPB_E_INVALID.
 * ------------------------------------------------------------------------------------------- */
int mpb_mesh_check(const float *mesh_host, int n_words);
int mpb_sdf_grid_build_mesh(const float *mesh, const float *pose_host, float *sdf, int flags, void *stream);

/* ---------------------------------------------------------------------------------------------
 * End effector: pose, geometric Jacobian, batched inverse kinematics (build-defined; the reference's Panda examples ask
 * torch_robotics' robot.get_EE_position, panda_spheres_GPMP.py:63-64).  Serial chains only (MPB_KIND_CHAIN): a point robot has no end
 * effector.
 *   pose:   the last frame of the chain walk, frame_{n_dof + 1} = [R | t], row-major 3 x 4 (the walk of mpb_fk_collision_points).
 *   J (6 x D), column j:  rows 0-2  z_j x (t - p_j),  rows 3-5  z_j   (z_j, p_j: axis and origin of joint j in the world).
 *   IK of a target (R*, t*) from a seed q0: damped least squares with a fixed budget.  At the start of each of n_iters iterations, and
 *   once more after the last step, the error is evaluated:
 *     e_p = t* - t;  E = R* R^T,  w = vee(E - E^T) / 2,  c = (tr E - 1) / 2,  theta = atan2(|w|, c),
 *     e_w = (theta / |w|) w, plain w when |w| < 1e-6 (exactly half a turn away the rotation part of the step is therefore zero).
 *   The problem is converged when |e_p| <= pos_tol and (theta <= rot_tol or position_only); a converged problem is frozen, its q is not
 *   touched again.  Otherwise one step:  dq = J^T (J J^T + damping^2 I)^{-1} e,  e = (e_p, e_w) -- with position_only e = e_p and the
 *   upper half of J --, then q <- clamp(q + dq, q_min, q_max), no clamp when the limits are not given.  No step-length cap, no line
 *   search, no null-space term.
 *   Bounds: 0 <= n_iters <= MPB_IK_MAX_ITERS, so a launch is bounded whatever the input, NaN included (a NaN problem never converges);
 *   damping >= MPB_IK_MIN_DAMPING: J J^T + damping^2 I is then SPD with condition number at most about 3e5 for chains of up to 12
 *   joints and reach up to about 1.2 m, which is what the unpivoted fp32 Cholesky of the kernel tolerates.
 *
 * geom: a packed geometry buffer in DEVICE memory, 16-byte aligned.  Only the first field's header (kind, n_dof, n_tf) and its joint_tf
 * section are read: no obstacle is touched and no geom_flags are needed.  The launchers read the header back ONCE per buffer address and
 * device (a synchronous 128-byte copy on the first call with that pointer -- make that call outside stream capture -- and again whenever
 * what was read does not fit the call's D); the kernels compare the header with the D they were launched with and answer NaN
 * (converged = 0) when it has changed since.
 *
 * mpb_fk_ee_pose: q (N, D) -> pose (N, 12); jac (N, 6, D) optional (may be NULL).  One lane per configuration.
 * mpb_ik_solve: target (N, 12), q_seed (N, S, D): S seeds per target; q_min, q_max (D each): both or neither (NULL).  Outputs per
 *   problem, all at the returned q: q_out (N, S, D), pos_err = |e_p| and rot_err = theta (N, S), converged (N, S) bytes 0 / 1,
 *   iters_used (N, S) = steps taken.  n_iters == 0 evaluates and steps nowhere: q_out is q_seed's bits.  One lane per (target, seed);
 *   no LDS, no atomics, no cross-lane arithmetic: a problem's bits depend on its own inputs only, and the pose the solver sees is the
 *   pose mpb_fk_ee_pose returns, bit for bit.  A wave leaves the iteration loop when all of its problems have converged.
 * Refusals, in this order: (1) D > MPB_MAX_DOF: MPB_E_UNSUPPORTED; (2) N < 0, D < 1 (solve: S < 0, N * S beyond an int, n_iters
 * outside 0..MPB_IK_MAX_ITERS, damping below MPB_IK_MIN_DAMPING or NaN, a negative or NaN tolerance): MPB_E_INVALID; (3) (N == 0 or S ==
 * 0: MPB_OK, nothing launched;) (4) a null required pointer, one of q_min / q_max without the other, geom not 16-byte aligned:
 * MPB_E_INVALID; then what only the header tells: bad magic / version: MPB_E_INVALID; (5) a point robot: MPB_E_UNSUPPORTED; (6) D !=
 * n_dof: MPB_E_INVALID.
 * ------------------------------------------------------------------------------------------- */
#define MPB_IK_MAX_ITERS 1024
#define MPB_IK_MIN_DAMPING 1e-2f
int mpb_fk_ee_pose(const float *q, const float *geom, float *pose, float *jac, int N, int D, void *stream);
int mpb_ik_solve(const float *target, const float *q_seed, const float *geom, const float *q_min, const float *q_max,
                 float *q_out, float *pos_err, float *rot_err, unsigned char *converged, int *iters_used,
                 int N, int S, int D, int n_iters, float damping, float pos_tol, float rot_tol, int position_only, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Cartesian end-effector moves: batched straight-line tracking (build-defined; what MoveIt calls computeCartesianPath).
 * Serial chains only; geom as for mpb_fk_ee_pose (the first field's header and joint_tf alone, the header read back once per address).
 * A problem is a pair (target n, start s): a goal pose [R* | t*], one per target and shared by its S starts, and a start configuration
 * q_0.  [R_0 | t_0] is the pose mpb_fk_ee_pose returns for q_0 (the kernel walks with the same routine and sees those bits).
 *   Once per problem, the rotation from R_0 to R* in the terms of mpb_ik_solve's error:  E = R* R_0^T,  w = vee(E - E^T) / 2,
 *     c = (tr E - 1) / 2,  theta = atan2(|w|, c),  axis a = w / |w|.  theta > MPB_CART_MAX_TURN (the geodesic is ill-conditioned near
 *     half a turn; a NaN angle counts): status MPB_CART_BAD_TARGET, n_ok = 0.  Otherwise theta is taken as 0 (no rotation) when
 *     |w| < 1e-6.  With position_only the rotation is ignored altogether: no angle is computed, no target is bad, rot_err is 0.
 *   Step k = 1 .. K, s_k = k / K:  t_k = t_0 + s_k (t* - t_0), evaluated as (1 - s_k) t_0 + s_k t* so that t_K is t* exactly;
 *     R_k = Rod(a, s_k theta) R_0,  Rod(a, phi) = cos(phi) I + sin(phi) [a]x + (1 - cos(phi)) a a^T, computed in the lane: nothing
 *     but the two end poses is read.
 *   From the last accepted configuration at most n_inner iterations, each exactly mpb_ik_solve's against [R_k | t_k]: the same error
 *     and tolerances, the same dq = J^T (J J^T + damping^2 I)^{-1} e, the same clamp onto q_min / q_max when given; a converged
 *     problem is frozen.  The error is evaluated once more after the last iteration.  Then
 *       not within (pos_tol, rot_tol):                      status MPB_CART_LOST, stop;
 *       else max_j |q_k[j] - q_{k-1}[j]| > jump_max:        status MPB_CART_JUMP, stop (the arm would change branch);
 *       else the step is accepted, n_ok = k.
 *   A problem that accepts all K steps has status MPB_CART_OK.  MPB_CART_COLLISION is never written by the library: it is the status
 *   of the callers that crop a path at its first colliding row (PlanningTask.cartesian_path).
 * Outputs per problem: q_path (N, S, K+1, D): row 0 is q_0's bits, row k <= n_ok the accepted configuration, every row beyond n_ok
 *   repeats row n_ok (always a valid trajectory, which holds still after the stop); pos_err, rot_err (N, S, K+1): the error of each
 *   accepted row against its step's target, 0 in row 0, the rejected step's errors in row n_ok + 1 (LOST and JUMP), 0 after that;
 *   n_ok (N, S) and status (N, S) int32.  When the geometry header has changed since the call: NaN in q_path (and the errors),
 *   n_ok = 0, status MPB_CART_LOST.
 * Bounds, so that a launch is bounded whatever the input, NaN included (a NaN problem never converges: it stops at step 1):
 *   1 <= K <= MPB_CART_MAX_STEPS, 0 <= n_inner <= MPB_IK_MAX_ITERS, K * n_inner <= MPB_CART_MAX_WORK, damping >= MPB_IK_MIN_DAMPING,
 *   jump_max > 0 (infinity turns the check off), tolerances not negative.  n_inner == 0 steps nowhere: a step is accepted only when
 *   its target is already within tolerance of the held pose.
 * One lane per problem; no LDS, no atomics, no cross-lane arithmetic: a problem's bits depend on its own inputs only.  A wave leaves
 * the loops when none of its problems needs them.
 * Refusals, in this order: (1) D > MPB_MAX_DOF: MPB_E_UNSUPPORTED; (2) N < 0, S < 0, D < 1, N * S beyond an int, K outside
 * 1..MPB_CART_MAX_STEPS, n_inner outside 0..MPB_IK_MAX_ITERS, K * n_inner beyond MPB_CART_MAX_WORK, damping below MPB_IK_MIN_DAMPING or
 * NaN, a negative or NaN tolerance, jump_max not positive or NaN: MPB_E_INVALID; (3) (N == 0 or S == 0: MPB_OK, nothing launched;)
 * (4) a null required pointer, one of q_min / q_max without the other, geom not 16-byte aligned: MPB_E_INVALID; then what only the
 * header tells: bad magic / version: MPB_E_INVALID; (5) a point robot: MPB_E_UNSUPPORTED; (6) D != n_dof: MPB_E_INVALID.
 * ------------------------------------------------------------------------------------------- */
#define MPB_CART_MAX_STEPS 4096
#define MPB_CART_MAX_WORK 65536
#define MPB_CART_MAX_TURN 3.04159265f /* pi - 0.1 */
#define MPB_CART_OK 0
#define MPB_CART_LOST 1
#define MPB_CART_JUMP 2
#define MPB_CART_BAD_TARGET 3
#define MPB_CART_COLLISION 4
int mpb_cartesian_path(const float *target, const float *q_start, const float *geom, const float *q_min, const float *q_max,
                       float *q_path, float *pos_err, float *rot_err, int *n_ok, int *status,
                       int N, int S, int D, int K, int n_inner, float damping, float pos_tol, float rot_tol, float jump_max,
                       int position_only, void *stream);

/* ---------------------------------------------------------------------------------------------
 * End-effector pose cost of a trajectory batch and its gradient (build-defined): the task-space term of the planners --
 * arrive at a pose, follow a Cartesian path, keep a tool axis (the cup upright) along the way.  Serial chains only; geom as for
 * mpb_fk_ee_pose (the first field's header and joint_tf alone, the header read back once per address, the kernels answer NaN when it has
 * changed since).  Per waypoint h of the range [h_begin, h_end), (R, t) the pose mpb_fk_ee_pose returns for trajs[b, h, :D] -- the
 * kernels walk the chain with the same routine and see those bits -- and [R* | t*] the waypoint's target:
 *   position term (k_pos > 0):            e_p = t* - t,  c_p = |e_p|^2
 *   rotation term, full (k_rot > 0, use_axis == 0):  e_w the rotation error of mpb_ik_solve above (E = R* R^T, w, c, theta = atan2(|w|,
 *            c), e_w = (theta / |w|) w, plain w below |w| = 1e-6),  c_r = |e_w|^2
 *   rotation term about one free tool axis (k_rot > 0, use_axis != 0): a = (ax, ay, az) a unit vector of the TOOL frame, u = R a,
 *            u* = R* a,  c_a = |u - u*|^2: the rotation about a is free, the cost is smooth everywhere
 *   c_h = k_pos c_p + k_rot (c_r or c_a);   out[b] (+)= weight * sum_{h_begin <= h < h_end} c_h
 *   gradient, DEFINED by the closed forms through J = (J_v; J_w) of mpb_fk_ee_pose:  d c_p / dq = -2 J_v^T e_p,
 *            d c_r / dq = -2 J_w^T e_w,  d c_a / dq = -2 J_w^T (u x u*).  The first and the last are exact derivatives; the second is
 *            the exact derivative of theta^2 for orthonormal R, R*, and theta = pi is a cut locus of c_r (a kink, like a hinge's edge).
 * A term with k = 0 is off; k = 1 / sigma^2 is the caller's.
 * target: ONE base pointer to poses of 12 words (row-major 3 x 4, as mpb_fk_ee_pose writes them); trajectory b at waypoint h reads pose
 *   (b / group) * stride_g + h * stride_h (strides in poses; either may be 0): one pose for all (0, 0), one per goal (1, 0; group =
 *   B / G trajectories per goal), one per waypoint (0, 1), both (H, 1).  The caller guarantees the poses those indices reach.
 * per_waypoint (B, H) optional: c_h, un-scaled by weight, 0 outside the range.  grad (B, H, d) (+)= d out[b] / d trajs[b]: without
 *   accumulate EVERY element is written (velocity channels D .. d-1 and rows outside the range 0); with accumulate the fresh value is
 *   added in ONE fp32 rounding onto out and onto the position channels of the range's rows, and nothing else is touched.
 * Two launch forms, chosen by the shape alone: a range of more than one waypoint runs one wave per trajectory, one lane per waypoint,
 *   trips of 64 (a lane sums its trips in ascending order, then a fixed-order wave reduction); a range of exactly one waypoint runs one
 *   lane per trajectory.  No LDS, no atomics: the same bits on every run.
 * Refusals, in this order, the first nine before any HIP call: D > MPB_MAX_DOF or d > 2 MPB_MAX_DOF: MPB_E_UNSUPPORTED; B < 0, H < 1,
 * D < 1, 64 H d beyond an int; d < D; a range outside 0 <= h_begin < h_end <= H; group < 1 or not dividing B; a negative stride; k_pos or
 * k_rot negative, NaN or infinite; both 0; use_axis with k_rot == 0 or with an axis whose length is not 1 within 1e-3: MPB_E_INVALID;
 * (B == 0: MPB_OK, nothing launched;) a null required pointer, geom not 16-byte aligned: MPB_E_INVALID; then what only the header
 * tells, as for mpb_fk_ee_pose: bad magic / version: MPB_E_INVALID; a point robot: MPB_E_UNSUPPORTED; D != n_dof: MPB_E_INVALID.
 * ------------------------------------------------------------------------------------------- */
int mpb_ee_cost_eval(const float *trajs, const float *geom, const float *target, float *out, float *per_waypoint,
                     int B, int H, int d, int D, int h_begin, int h_end, int group, int stride_g, int stride_h,
                     float k_pos, float k_rot, int use_axis, float ax, float ay, float az, float weight, int accumulate, void *stream);
int mpb_ee_cost_grad(const float *trajs, const float *geom, const float *target, float *out, float *grad,
                     int B, int H, int d, int D, int h_begin, int h_end, int group, int stride_g, int stride_h,
                     float k_pos, float k_rot, int use_axis, float ax, float ay, float az, float weight, int accumulate, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Batched RRT-Connect -- replaces RRTConnect._run_optimization (rrt_connect.py:93-192) with RRTBase.get_pre_sample /
 * remove_last_pre_sample / get_nearest_node (rrt_base.py:59-63, :94-98, :115-119), extend_path, safe_path and
 * purge_duplicates_from_traj (utils.py:4-50), for B independent problems at once (what MultiSampleBasedPlanner fans out
 * over a process pool).  One persistent launch, one workgroup per problem; workgroups never wait on each other.
 *
 * workspace: mpb_rrt_connect_workspace_bytes(B, max_nodes, n_pre, D) bytes, 16-byte aligned (0 = shape refused, see
 *   mpb_last_error).  The layout in numbers is mpb_rrt_layout.h (generated from rrt_layout.py, the one definition); in
 *   32-bit words: MPB_RRT_GLOBAL_WORDS words, of which MPB_RRTG_MAGIC (MPB_RRT_CONNECT_MAGIC), _B, _MAX_NODES, _N_PRE,
 *   _D and _DP (D rounded up to 4) are used; B x MPB_RRT_CONNECT_HDR_WORDS words per problem, of which
 *   MPB_RRTC_STATUS (MPB_RRT_*), _ITERS (iterations used), _COUNTS (two words: nodes of tree 0, nodes of tree 1), _SWAP
 *   (the swap bit) and _POOL_LEN are used;
 *   node configurations (B, 2, max_nodes, Dp) fp32, zero padded; parents (B, 2, max_nodes) int32 (-1: root);
 *   pool lists (B, (n_pre + 1) / 2) words of two uint16 indices into pre_samples.  Tree 0 is rooted at the start, tree 1
 *   at the goal; the reference's name swap is the swap bit (`continue` leaves an iteration before the swap-back, so a
 *   returned path may run goal -> start).
 * mpb_rrt_connect_init: roots, counts, the full pool list 0 .. n_pre - 1, and the start / goal collision check
 *   (rrt_connect.py:100-101: status START_OR_GOAL_IN_COLLISION, no path).  start, goal (B,D).
 * mpb_rrt_connect_run: iterations iter0 .. min(iter0 + n_iters, total_iters) - 1 of every problem still RUNNING, resumed
 *   from the workspace (call in chunks with iter0 advancing; a problem that reaches total_iters becomes EXHAUSTED_ITERS).
 *   pre_samples: the pool, (n_pre, D) shared by all problems (pre_stride = 0) or one per problem (pre_stride = floats
 *   between two problems' pools).  sample_idx: NULL -> the index of the iteration's target in the CURRENT pool list is
 *   mulhi(Philox4x32-10(counter = (problem_offset + b, iteration, tag, 0), key = seed).x, pool length); else
 *   (B, total_iters) int32 recorded indices (the reference's torch.randperm(len(pool))[0]), clamped to the list.
 *   One index per iteration, also in iterations that `continue`.  A reached target (allclose) is deleted from the list,
 *   order kept; an empty list ends the problem with POOL_EMPTY (refilling is not served on the device).
 *   paths (B,Lmax,D), lengths (B): the purged path and its node count for FOUND problems (the layout mpb_traj_resample
 *   takes); PATH_TOO_LONG when the un-purged path has more than Lmax nodes.  status (B): copy of the status words.
 *   A tree that would exceed max_nodes ends with TREE_FULL (max_nodes >= total_iters + 1 cannot).
 * ------------------------------------------------------------------------------------------- */
/* MPB_RRT_* (the status values) and MPB_RRT_MAX_PRE_SAMPLES: mpb_rrt_layout.h */
size_t mpb_rrt_connect_workspace_bytes(int B, int max_nodes, int n_pre, int D);
int mpb_rrt_connect_init(void *workspace, size_t workspace_bytes, const float *start, const float *goal,
                         const float *geom, int geom_flags, int B, int max_nodes, int n_pre, int D, void *stream);
int mpb_rrt_connect_run(void *workspace, size_t workspace_bytes, const float *geom, int geom_flags,
                        const float *pre_samples, size_t pre_stride, const int *sample_idx, float *paths,
                        int *lengths, int *status, int B, int max_nodes, int n_pre, int D, int Lmax, int iter0,
                        int n_iters, int total_iters, float step_size, float n_radius, uint64_t seed,
                        uint32_t problem_offset, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Space-time RRT-Connect among moving obstacles (build-defined: the reference has nothing like it) for B independent problems
 * at once.  One persistent launch, one single-wave workgroup per problem; workgroups never wait on each other, there is no
 * spin wait, every loop is bounded by n_iters, max_nodes, n_rows or Lmax, and a finished problem returns at once.
 *
 * Time lives on the row grid of a packed moving-obstacle buffer `moving` (mpb_moving_layout.h) packed for n_rows = R rows,
 *   MPB_STRRT_MIN_ROWS <= R <= MPB_STRRT_MAX_ROWS: row h is the field's time t_start + h (t_end - t_start) / (R - 1).  Obstacle
 *   positions are never interpolated: every check is made AT A ROW with the buffer's centres of that row, the statement
 *   mpb_moving_collision_check makes of a trajectory.  A finer clock is a larger R.
 * Problem b: start (b) at row 0, goal (b) at row R - 1; w (D): the most joint k may move per row, fp32(dq_max_k * dt_row).
 * Predicate of (q, row): the static cost of geom (chained fields, as mpb_collision_check) is positive OR the moving cost of
 *   that row (as mpb_moving_collision_check) is.
 * Tree: nodes (q, row, parent); tree 0 is rooted at (start, 0) and grows forward in time (a child's row is greater than its
 *   parent's), tree 1 at (goal, R - 1) and grows backward.  Waiting is an ordinary edge with little or no motion.
 * Metric from node n to a target (q_r, h_r) on the tree's growing side, dh = |h_r - h_n| >= 1:
 *   tau = max_k (|q_r[k] - q_n[k]| / w_k), m = max(tau, (float)dh); nearest = least m, lowest index on ties.
 * Extension from n: s = min(dh, max_step_rows) rows (a connect target: s = dh); f = tau > dh ? dh / tau : 1;
 *   dl = (q_r - q_n) * f; point j (1 <= j <= s) = fma(dl, (float)j / (float)dh, q_n) at row h_n +- j; point j = dh with f == 1
 *   is q_r's own bits.  The first colliding point j0 == 1 fails the extension; otherwise point j0 - 1 (or s) is appended.
 * Iteration it: tree it & 1 extends towards (pre_samples[idx], row): sample_idx / sample_row NULL -> idx = mulhi(x, n_pre),
 *   row = 1 + mulhi(y, R - 2) of Philox4x32-10(counter = (problem_offset + b, it, MPB_STRRT_MAGIC, 0), key = seed); else
 *   (B, total_iters) int32 recorded draws, clamped to 0 .. n_pre - 1 and 1 .. R - 2.  Then the other tree extends towards
 *   the new node; when it appends that very node (same row, every coordinate allclose, and arrived at with f == 1: an allclose
 *   near miss with tau slightly above dh would put an edge faster than w into the plan) the trees are joined: vertices = tree
 *   0's chain from its root to its new node, then tree 1's chain from the PARENT of its new node to its root; the dense
 *   trajectory is fma(q_b - q_a, (float)(h - h_a) / (float)(h_b - h_a), q_a) between consecutive vertices, the vertex rows
 *   their own bits; every one of the R rows is then checked again.  A failing row discards the join (MPB_STH_REJECTED_JOINS
 *   goes up, the search continues); otherwise FOUND: every row of the output is free by the kernel's own predicate.
 * workspace: mpb_strrt_workspace_bytes(B, max_nodes, D) bytes, 16-byte aligned (0 = shape refused).  mpb_strrt_layout.h
 *   (generated from strrt_layout.py): MPB_STRRT_GLOBAL_WORDS words -- MPB_STG_MAGIC, _B, _MAX_NODES, _D, _DP (D rounded up to
 *   4), _N_ROWS --; per problem MPB_STRRT_HDR_WORDS words -- MPB_STH_STATUS (MPB_STRRT_*), _ITERS (iterations begun), _COUNTS
 *   (two words: nodes of tree 0, of tree 1), _REJECTED_JOINS --; then nodes (B, 2, max_nodes, Dp) fp32 zero padded, rows
 *   (B, 2, max_nodes) int32, parents (B, 2, max_nodes) int32 (-1: root).
 * mpb_strrt_init: roots, counts, status: START_OR_GOAL_IN_COLLISION (start at row 0, goal at row R - 1), else
 *   HORIZON_TOO_SHORT when tau(goal, start) > R - 1, else RUNNING.
 * mpb_strrt_run: iterations iter0 .. min(iter0 + n_iters, total_iters) - 1 of every problem still RUNNING, resumed from the
 *   workspace.  trajs (B,R,D); vertex_q (B,Lmax,D), vertex_row (B,Lmax), n_vertices (B): written for FOUND problems (trajs may
 *   hold the rows of a discarded join otherwise); more than Lmax vertices: PATH_TOO_LONG; a full tree: TREE_FULL; total_iters
 *   used up: EXHAUSTED_ITERS.  status (B): copy of the status words.  log: NULL or (B, total_iters, MPB_STRRT_LOG_WORDS) int32
 *   the caller has filled with MPB_STRRT_LOG_NONE: per iteration the extension towards the sample at word 0 and the connect
 *   extension at word MPB_STRRT_LOG_EXT_WORDS, each MPB_STL_TREE, _NEAREST, _DH, _S, _FIRST (first colliding point or -1),
 *   _APPENDED (node index or -1), and at word MPB_STRRT_LOG_JOIN the first failing row of a join's re-check or -1.
 * Refusals: D > MPB_MAX_DOF, n_rows > MPB_STRRT_MAX_ROWS: MPB_E_UNSUPPORTED; n_rows < MPB_STRRT_MIN_ROWS, bad shapes, null
 *   pointers, misaligned buffers, a small workspace, one recorded-draw array without the other: MPB_E_INVALID; then the moving
 *   buffer's header (through the cache mpb_moving_invalidate serves): n_rows and n_dof must equal the call's, and the message
 *   names both numbers.
 * ------------------------------------------------------------------------------------------- */
size_t mpb_strrt_workspace_bytes(int B, int max_nodes, int D);
int mpb_strrt_init(void *workspace, size_t workspace_bytes, const float *start, const float *goal, const float *w,
                   const float *geom, int geom_flags, const float *moving, int B, int max_nodes, int D, int n_rows, void *stream);
int mpb_strrt_run(void *workspace, size_t workspace_bytes, const float *geom, int geom_flags, const float *moving, const float *w,
                  const float *pre_samples, size_t pre_stride, const int *sample_idx, const int *sample_row, float *trajs,
                  float *vertex_q, int *vertex_row, int *n_vertices, int *status, int *log, int B, int max_nodes, int n_pre, int D,
                  int n_rows, int Lmax, int max_step_rows, int iter0, int n_iters, int total_iters, uint64_t seed,
                  uint32_t problem_offset, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Timing of geometric paths among moving obstacles: path-velocity decomposition (build-defined, DESIGN.md 10: the reference has
 * nothing like it).  N paths of S samples each keep their shape; each gets the rows of the clock at which to stand on which sample --
 * advancing or waiting, never going back -- so that every row is free at its own time.  One workgroup per path, no workspace.
 *
 * paths (N, S, D) fp32: sample 0 the start, sample S - 1 the goal; MPB_PT_MIN_SAMPLES <= S <= MPB_PT_MAX_SAMPLES.  The clock is the row
 *   grid of `moving` (mpb_moving_layout.h) packed for n_rows = R rows, MPB_PT_MIN_ROWS <= R <= MPB_PT_MAX_ROWS: the clock of
 *   mpb_strrt_run and mpb_moving_collision_check.  w (D): the most joint k may move per row, fp32(dq_max_k * dt_row), finite and positive.
 *   blocked: NULL or (N, S) bytes, nonzero = the sample is refused by a static predicate of the caller's.
 * 1 segment cost   c_i = max over k of fl(fl(|fl(P[i+1,k] - P[i,k])|) / w_k), starting from 0, every operation rounded, none contracted
 *                  (the tau of mpb_strrt_run); cfix_i = (uint32) ceilf(c_i * MPB_PT_COST_ONE).  A term above 1 or not finite:
 *                  MPB_PT_SEGMENT_TOO_LONG -- no single row can cross that segment, resample the path more densely.
 * 2 prefix sums    C_i = sum of cfix_m over m < i, in integers (at most 255 * MPB_PT_COST_ONE).
 * 3 advance rule   in one row from sample i to sample i' >= i iff C_i' - C_i <= MPB_PT_COST_ONE (waiting: i' = i).  The sum of the
 *                  per-segment maxima bounds every joint's travel along the polyline, so a row step moves joint k by at most w_k up to
 *                  fp32 rounding: the plan definition of mpb_strrt_run.  lo_i' = the smallest i the rule admits.
 * 4 free table     F[j][i] = !blocked[i] && !(the predicate of mpb_moving_collision_check for P[i] at row j), the buffer's centres of
 *                  row j; nothing is interpolated between rows.
 * 5 reachability   reach[0][i] = (i == 0) && F[0][0];  reach[j][i'] = F[j][i'] && OR over i in [lo_i', i'] of reach[j-1][i].
 * 6 arrival        hold[j] = F[j'][S-1] for every j' >= j; the arrival row j* = the least j with reach[j][S-1] && hold[j].
 * 7 backtrack      idx[j*] = S - 1; for j = j* .. 1: idx[j-1] = the largest i in [lo_idx[j], idx[j]] with reach[j-1][i]; idx[j] = S - 1
 *                  for j > j* (held at the goal).
 * 8 output         trajs (N, R, D): row j = P[idx[j]], the sample's own bits; all zero where no timing was found.
 * 9 status (N)     MPB_PT_FOUND, or the first that applies of MPB_PT_BUFFER_CHANGED (the header of `moving` differs from what the
 *                  launcher read -- through the cache mpb_moving_invalidate serves --: nothing of it is trusted, the table reads all
 *                  zero), MPB_PT_SEGMENT_TOO_LONG, MPB_PT_START_BLOCKED (!F[0][0]), MPB_PT_GOAL_NOT_HOLDABLE (!F[R-1][S-1]), MPB_PT_NO_TIMING.
 * Exact on this lattice: MPB_PT_FOUND arrives at the earliest row any monotone timing under the advance rule can; MPB_PT_NO_TIMING
 * means none exists on it.  No random draws; every run gives the same bits.
 * Optional outputs (NULL: not written): idx (N, R) int32, -1 where no timing was found; arrival_row (N) int32, -1 likewise; free_table
 *   (N, R, S) bytes, F as above (with MPB_PT_SEGMENT_TOO_LONG the table is evaluated only when it is asked for).
 * Not built: backward motion along the path, obstacle interpolation between rows, acceleration limits, arrival trade-offs other than
 *   the earliest row.
 * Refusals: D > MPB_MAX_DOF, S > MPB_PT_MAX_SAMPLES, n_rows > MPB_PT_MAX_ROWS, shapes beyond 2e9 elements: MPB_E_UNSUPPORTED; S or n_rows
 *   below their minimum, bad shapes, (N > 0:) a null required pointer, a moving buffer not 16-byte aligned: MPB_E_INVALID; the buffer's
 *   header: n_rows and n_dof must equal the call's, the message names both numbers; an LDS need -- MPB_PT_LDS_WORDS of the robot's
 *   collision spheres, S and n_rows, in 32-bit words -- above MPB_PT_MAX_LDS_BYTES: MPB_E_UNSUPPORTED, by that name.
 * ------------------------------------------------------------------------------------------- */
int mpb_path_time_plan(const float *paths, const float *moving, const float *w, const unsigned char *blocked, float *trajs,
                       int *idx, int *arrival_row, int *status, unsigned char *free_table, int N, int S, int D, int n_rows,
                       void *stream);

/* ---------------------------------------------------------------------------------------------
 * Space-time shortcutting: the pass between a planner on the moving-obstacle clock (mpb_strrt_run, mpb_path_time_plan) and the
 * optimiser (build-defined, DESIGN.md 10: the reference has nothing like it).  N dense trajectories keep their row count -- and so their
 * clock --; an iteration replaces the rows BETWEEN two rows by the constant-velocity straight piece, and keeps the replacement only when
 * every new row is free at its own time and the piece respects the per-row velocity bound.  One single-wave workgroup per trajectory,
 * the trajectory in LDS for the whole launch, no workspace.
 *
 * trajs_in (N, R, D) fp32, MPB_STS_MIN_ROWS <= R <= MPB_STS_MAX_ROWS, finite; trajs_out (N, R, D), may be trajs_in (in place).  geom: the
 *   packed geometry of the static scene (chained fields allowed), geom_flags its mpb_geom_flags.  moving: a packed moving-obstacle buffer
 *   for n_rows = R (mpb_moving_layout.h): row h is seen at the time of the buffer's row h.  w (D): the most joint k may move per row,
 *   fp32(dq_max_k * dt_row) as mpb_strrt_run takes it, finite and positive.  valid: NULL or (N) bytes, 0 = pass the trajectory through.
 *   draws: NULL or (N, n_iters, 2) int32 recorded rows.  max_span: 0 (no limit) or the most rows a piece may span.
 * 1 predicate      of (q, row): the static cost of geom is positive (the predicate of mpb_collision_check) OR the moving cost of that
 *                  row is (the predicate of mpb_moving_collision_check): the predicate of mpb_strrt_run, exactly.  Rows are checked at
 *                  the rows only; obstacle positions are never interpolated.
 * 2 input gate     per trajectory, before any iteration: all R rows by the predicate, then every step
 *                  tau(q[h+1], q[h]) <= MPB_STS_GATE_LIMIT = 1 + 2^-16, tau(x, y) = max over k of fl(fl(|fl(x_k - y_k)|) / w_k) from 0
 *                  (the tau of mpb_strrt_run).  The slack is derived: both producers keep every step within w (1 + 1e-5), tau's own three
 *                  roundings add under 2e-7, 2^-16 = 1.53e-5 clears the sum.
 * 3 status (N)     the first that applies of MPB_STS_NOT_VALID (valid[n] == 0), MPB_STS_BUFFER_CHANGED (the header of `moving` differs
 *                  from what the launcher read -- through the cache mpb_moving_invalidate serves --: nothing of it is read),
 *                  MPB_STS_INPUT_IN_COLLISION, MPB_STS_INPUT_TOO_FAST; else MPB_STS_OK.  first_bad (N): the first colliding row, or
 *                  the row h + 1 of the first step h -> h + 1 above the limit; else -1.  Only MPB_STS_OK trajectories are edited: every
 *                  other one comes out with its input bits.
 * 4 draws          iteration `it` of trajectory n: ONE Philox4x32-10 call, counter (problem_offset + n, it, MPB_STS_PHILOX_TAG, 0),
 *                  key = seed; r0 = mulhi(x, R), r1 = mulhi(y, R).  Recorded draws: the two ints clamped into 0 .. R - 1.
 *                  a = min(r0, r1), b = max(r0, r1); with max_span > 0: b = min(b, a + max_span).
 * 5 decisions      in this order: b - a < 2: MPB_STS_LOG_SKIP_SHORT.  tau(q_b, q_a) > (float)(b - a): MPB_STS_LOG_SKIP_FAST (the
 *                  f == 1 condition of mpb_strrt_run's steering: the filled rows obey the rounding argument of its fill).  Candidate
 *                  row h, a < h < b: fma(q_b - q_a, (float)(h - a) / (float)(b - a), q_a) -- the subtraction and the division rounded,
 *                  ONE fused multiply-add: the dense-row expression of mpb_strrt_run, bit for bit; rows a and b keep their bits.  Every
 *                  candidate row within |c - o| <= fma(1e-5, |o|, 1e-8) of the row o it would replace, in every coordinate:
 *                  MPB_STS_LOG_SKIP_STRAIGHT, nothing is evaluated.  Rows a + 1 .. b - 1 by the predicate at their own rows, ascending: a
 *                  hit is MPB_STS_LOG_REJECT | first colliding row << MPB_STS_LOG_INDEX_SHIFT.  Otherwise MPB_STS_LOG_ACCEPT: the
 *                  candidate rows replace the old ones.  Rows 0 and R - 1 never change.
 * 6 outputs        stats (N, 4) fp32: candidates checked (REJECT + ACCEPT), accepted, joint-space length before, after -- per-row
 *                  distances, the squares summed in index order with every operation rounded, square-rooted and summed in row order --;
 *                  NaN where the trajectory is not MPB_STS_OK.  log: NULL or (N, n_iters) int32, one word per iteration as above,
 *                  MPB_STS_LOG_IDLE where the trajectory is not MPB_STS_OK.
 * No atomics, a fixed order: the same bits on every run; a trajectory's bits depend on its own inputs only.
 * Guarantee: an MPB_STS_OK output is free on every row by the predicate above; starts and ends on the input's bits; every step the pass
 *   wrote is within w_k (1 + 1e-5) (a step of a piece is |q_b - q_a| / (b - a) <= w up to the roundings of tau, the division and the
 *   fma); and its fp64 length is no longer than the input's up to rounding: a candidate row differs per coordinate from the exact chord
 *   point by at most 6 * 2^-24 * M (the rounded difference and quotient, the fma's one rounding; M the largest |coordinate| of the input),
 *   the exact chord is no longer than the rows it replaces, and a row moved by e lengthens its two steps by at most 2 e, so
 *   len(out) <= len(in) + 2 W * 6 * 2^-24 * sqrt(D) * M with W the rows written, at most accepted * (R - 2).
 * Not built: self_field / sdf_field members in the predicate, obstacle interpolation between rows, acceleration limits, changing the
 *   arrival row, per-joint shortcutting, cost-aware acceptance.
 * Refusals: D > MPB_MAX_DOF, n_rows > MPB_STS_MAX_ROWS, shapes beyond 2e9 elements: MPB_E_UNSUPPORTED; n_rows < MPB_STS_MIN_ROWS, bad
 *   shapes, n_iters outside 0 .. MPB_STS_MAX_ITERS, max_span < 0, (N > 0:) a null required pointer, geom or moving not 16-byte aligned:
 *   MPB_E_INVALID; the buffer's header: n_rows and n_dof must equal the call's, the message names both numbers; an LDS need --
 *   MPB_STS_LDS_BYTES(n_rows, D) -- above MPB_STS_MAX_LDS_BYTES: MPB_E_UNSUPPORTED, by that name.
 * ------------------------------------------------------------------------------------------- */
int mpb_st_shortcut(const float *trajs_in, float *trajs_out, const float *geom, int geom_flags, const float *moving, const float *w,
                    const unsigned char *valid, const int *draws, int *status, int *first_bad, float *stats, int *log, int N,
                    int n_rows, int D, int n_iters, int max_span, uint64_t seed, uint32_t problem_offset, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Batched RRT* and informed RRT* -- replaces RRTStar._run_optimization (rrt_star.py:133-261) with OptimalNode's cost
 * bookkeeping (:16-61), RRTBase.get_pre_sample / remove_last_pre_sample / get_nearest_node (rrt_base.py:59-63, :94-98,
 * :115-119), extend_path, safe_path and purge_duplicates_from_traj (utils.py:4-50), for B independent problems at once.
 * One persistent launch, one single-wave workgroup per problem; workgroups never wait on each other.  Only the radius
 * neighbourhood (n_knn == 0) is served.
 *
 * workspace: mpb_rrt_star_workspace_bytes(B, max_nodes, n_pre, D) bytes, 16-byte aligned (0 = shape refused, see
 *   mpb_last_error).  In 32-bit words: the MPB_RRT_GLOBAL_WORDS words of mpb_rrt_connect's workspace with
 *   MPB_RRT_STAR_MAGIC; B x MPB_RRT_STAR_HDR_WORDS words per problem, of which these are used: MPB_RRTS_STATUS,
 *   _ITERS (loop bodies started: the reference's final `iteration` + 1), _COUNT (nodes), _GOAL (index of the goal node,
 *   -1: none), _POOL_LEN, _STOP_REASON (MPB_RRT_STOP_*), _BEST_COST_ITERS, _ITERS_AFTER_FIRST_SUCCESS, _BEST_COST_EPS
 *   (fp32 bits; 3e38 before the first success), _REWIRES (accepted), _INFORMED_REJECTIONS, _FIRST_COST (goal cost at the
 *   first success, fp32 bits), _FIRST_ITER (iteration of the first success, -1: none), _FIRST_COUNT (node count at the
 *   first success: nodes from this index on were created after the goal node);
 *   goal configurations (B, Dp) fp32; ONE tree per problem, rooted at the start: node configurations (B, max_nodes, Dp)
 *   fp32, zero padded; parents (B, max_nodes) int32 (-1: root; after a rewire a parent may follow its child); d
 *   (B, max_nodes) fp32, the length of the edge to the parent; cost (B, max_nodes) fp32 with
 *   cost[i] == fl32(cost[parent[i]] + d[i]) bitwise, root 0; neighbour scratch (B, 3, max_nodes) (rewire candidates of
 *   the current iteration: index, d, edge verdict); pool lists (B, (n_pre + 1) / 2) words of two uint16 indices.
 * mpb_rrt_star_init: root, goal, counters, the full pool list 0 .. n_pre - 1, and the start / goal collision check
 *   (rrt_star.py:143-144: status START_OR_GOAL_IN_COLLISION, no path).  start, goal (B,D).
 * mpb_rrt_star_run: loop bodies iter0 .. min(iter0 + n_iters, total_iters) - 1 of every problem still RUNNING, resumed
 *   from the workspace (call in chunks with iter0 advancing; total_iters = the reference's n_iters + 1).  Per body, in
 *   the reference's order: (:167-168) best_cost_iters >= max_best_cost_iters stops (COST_CONVERGED); (:169-174) with a
 *   goal node, goal cost < best_cost_eps - cost_eps (fp32) resets best_cost_iters, else counts it; (:176-182)
 *   iters_after_first_success > n_iters_after_success stops (AFTER_SUCCESS; n_iters_after_success < 0 = None);
 *   (:185) goal draw iff no goal node exists and (iteration == 0 or uniform < goal_prob), else a pool entry;
 *   (:197-199) informed != 0 and a goal node exists and d(start, s) + d(s, goal) >= goal cost: the entry is deleted,
 *   the body ends; (:202-208) nearest node, extend_path, safe_path as in mpb_rrt_connect_run; (:210-211) a sample the
 *   extension reached (allclose) is deleted; (:213-222) the new node with d and cost, the goal node iff this was a goal
 *   draw and d(new, goal) < eps; (:225-251) every node within n_radius whose cost the new node lowers and whose edge
 *   from the new node is free up to eps is rewired in index order, the costs of its subtree following before the next
 *   neighbour is tested.
 *   pre_samples, pre_stride as in mpb_rrt_connect_run.  sample_idx, goal_draw: both NULL -> one Philox4x32-10 call per
 *   (problem, iteration) (counter = (problem_offset + b, iteration, tag, 0), key = seed): .x gives the pool index by
 *   mulhi with the pool length, the top 24 bits of .y the uniform compared with goal_prob in fp32; else both
 *   (B, total_iters) int32: goal_draw 1 = goal, 0 = sample (iteration 0 always aims at the goal; ignored once a goal
 *   node exists), sample_idx the recorded torch.randperm(len(pool))[0], clamped, ignored where the goal is drawn.
 *   At the end of EVERY launch a problem that has a goal node gets its current retrace root -> goal through
 *   purge_duplicates_from_traj in paths (B,Lmax,D) / lengths (B) and the goal's cost in costs (B), so a run cut between
 *   chunks still returns its best path.  status (B): copy of the status words: FOUND iff a goal node exists when the
 *   problem stops (why it stopped: stop_reason), else EXHAUSTED_ITERS (also for the two early stops without a goal
 *   node), POOL_EMPTY (a sample was needed from an empty list), TREE_FULL (max_nodes >= total_iters + 1 cannot),
 *   PATH_TOO_LONG (the un-purged retrace has more than Lmax nodes; lengths 0).
 * Refusals: n_pre > MPB_RRT_MAX_PRE_SAMPLES, D > MPB_MAX_DOF, B x max_nodes beyond 32-bit indexing: MPB_E_UNSUPPORTED;
 *   null pointers (sample_idx / goal_draw given one without the other included), misaligned workspace / geom, a short
 *   workspace, Lmax < 2, a bad iteration range, non-positive step_size / n_radius: MPB_E_INVALID.
 * ------------------------------------------------------------------------------------------- */
/* stop_reason (MPB_RRT_STOP_* of mpb_rrt_layout.h): RUNNING; ITERS, the n_iters + 1 loop bodies are used up;
 * COST_CONVERGED, best_cost_iters >= max_best_cost_iters; AFTER_SUCCESS, iters_after_first_success >
 * n_iters_after_success; TREE_FULL, a FOUND problem whose tree reached max_nodes; POOL_EMPTY, a FOUND problem whose
 * pool list ran empty */
size_t mpb_rrt_star_workspace_bytes(int B, int max_nodes, int n_pre, int D);
int mpb_rrt_star_init(void *workspace, size_t workspace_bytes, const float *start, const float *goal,
                      const float *geom, int geom_flags, int B, int max_nodes, int n_pre, int D, void *stream);
int mpb_rrt_star_run(void *workspace, size_t workspace_bytes, const float *geom, int geom_flags,
                     const float *pre_samples, size_t pre_stride, const int *sample_idx, const int *goal_draw,
                     float *paths, int *lengths, float *costs, int *status, int B, int max_nodes, int n_pre, int D,
                     int Lmax, int iter0, int n_iters, int total_iters, int max_best_cost_iters,
                     int n_iters_after_success, int informed, float step_size, float n_radius, float goal_prob,
                     float cost_eps, float eps, uint64_t seed, uint32_t problem_offset, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Batched path shortcutting -- the pass between the tree and the optimiser (pybullet-planning's smooth_path, OMPL's
 * PathSimplifier; the reference did not carry it over: build-defined).  One launch, one single-wave
 * workgroup per path, the path in LDS; no atomics and a fixed order: the same bits on every run, and a path's bits depend
 * on its own inputs only.
 * paths_in (N,Lmax,D), lengths_in (N): the batch mpb_rrt_*_run writes and mpb_traj_resample reads.  paths_out, lengths_out:
 *   the edited batch; paths_out == paths_in is allowed (in place; otherwise the two do not overlap).  Rows at and past a
 *   path's length are written as zeros.  The first and the last row of a path keep their input bits.  A path of fewer than
 *   3 nodes passes through; lengths_in[b] outside 0 .. Lmax: lengths_out[b] = 0, NaN in all four stats, a zeroed path.
 * A path of current length L >= 3 runs n_iters iterations; iteration i:
 *   draws u1, u2 in [0,1): draws == NULL -> one Philox4x32-10 call (counter = (problem_offset + b, i, tag, 0), key = seed;
 *     the tag is this entry point's own), u = (top 24 bits of .x, .y) * 2^-24; else (N, n_iters, 2) fp32 recorded draws,
 *     clamped into [0,1), NaN read as 0.
 *   position of a draw: s = fl32(u * (float)(L-1)), a = min((int)s, L-2), t = s - (float)a; the two ordered so that
 *     (a1,t1) <= (a2,t2).  a1 == a2: SKIP.
 *   point of a position: q_a + t * (q_{a+1} - q_a), rounded after each operation (no fma).  t == 0, or a point allclose
 *     (torch.allclose's defaults, the point against the node) to node a, IS node a; else a point allclose to node a+1 is
 *     that node.  With lo the last node at or before point 1 and hi the first node at or after point 2: hi - lo < 2
 *     (both on one segment) or the two points allclose: SKIP.
 *   candidate P1 -> P2: checked as mpb_rrt_connect_run checks an extension, without its n_radius clamp: dist the
 *     sequential fp32 sum in index order, n_pts = (int)(dist / check_step) + 2 points of extend_path's linspace (more than
 *     2^20: SKIP), a point in collision iff mpb_collision_check says so; the scan stops after the 64 points that hold the
 *     first hit.  A hit: REJECT with the index of the first point in collision.
 *   free: nodes lo+1 .. hi-1 are replaced by the points that are no nodes (0, 1 or 2 rows), ACCEPT; unless the new length
 *     would exceed Lmax (one node replaced by two on a full path): OVERFLOW, nothing changes.
 * stats (N,4) fp32: candidates checked (REJECT + OVERFLOW + ACCEPT), accepted, the joint-space length before and after
 *   (the distances above summed in fp32 in path order).  log (N,n_iters) int32, optional (may be NULL):
 *   MPB_SHORTCUT_* | (first index << MPB_SHORTCUT_LOG_INDEX_SHIFT); IDLE: the path had fewer than 3 nodes.
 * Refusals, in this order, all before the first HIP call: D > MPB_MAX_DOF: MPB_E_UNSUPPORTED; N < 0 or D < 1; Lmax < 2 or
 *   4 * Lmax * Dp bytes (Dp = D rounded up to 4) beyond the 160 KB of LDS less the 17 408 bytes of the staged grid -- Lmax
 *   at most 9152 / 4576 / 3050 for Dp = 4 / 8 / 12; n_iters < 0 or > MPB_SHORTCUT_MAX_ITERS; check_step not finite or <= 0;
 *   a null required pointer; geom not 16-byte aligned: MPB_E_INVALID.  N == 0: MPB_OK, nothing launched; n_iters == 0:
 *   MPB_OK, the outputs are a copy (stats: 0, 0, length, length).  Nothing more is refused: geom is device memory.
 * ------------------------------------------------------------------------------------------- */
#define MPB_SHORTCUT_IDLE 0
#define MPB_SHORTCUT_SKIP 1
#define MPB_SHORTCUT_REJECT 2
#define MPB_SHORTCUT_OVERFLOW 3
#define MPB_SHORTCUT_ACCEPT 4
#define MPB_SHORTCUT_LOG_INDEX_SHIFT 8
#define MPB_SHORTCUT_MAX_ITERS 1048576
int mpb_path_shortcut(const float *paths_in, const int *lengths_in, float *paths_out, int *lengths_out,
                      float *stats, int *log, const float *geom, int geom_flags, const float *draws,
                      int N, int Lmax, int D, int n_iters, float check_step,
                      uint64_t seed, uint32_t problem_offset, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Batched PRM -- one roadmap of collision-free configurations, many start / goal queries (the reference has no roadmap
 * planner: build-defined).  Three launches: the K nearest nodes, the edges' segment scans, the queries.
 * Arithmetic shared by all three, rounded after every operation (no fma): d2(x, y) the sequential fp32 sum over the joints
 * in index order of fl(fl(x_k - y_k)^2); dist = sqrtf(d2), the distance of the shortcut pass above.
 *
 * mpb_prm_knn: queries (Q,D), nodes (M,D) -> idx (Q,K) int32, dist (Q,K) fp32: row i holds the K nodes of smallest d2 to
 *   query i in ascending order of (d2, index); a NaN d2 orders as +inf (and is written as +inf).  exclude_self != 0: the
 *   queries ARE the nodes (Q == M) and node i is left out of row i.
 *   Refusals, in this order, before the first HIP call: Q < 0 or D < 1: MPB_E_INVALID; D > MPB_MAX_DOF, M >
 *   MPB_PRM_MAX_NODES, K > MPB_PRM_MAX_K: MPB_E_UNSUPPORTED; M < 2; exclude_self with Q != M; K < 1 or K > M - (1 with
 *   exclude_self); a null pointer: MPB_E_INVALID.  Q == 0: MPB_OK, nothing launched.
 *
 * mpb_prm_edge_check: pts (P,D), pairs (E,2) int32 -> flag (E) int32, first (E) int32.  Pair (a,b) is scanned from point
 *   min(a,b) to point max(a,b) -- (a,b) and (b,a) give the same bits -- exactly as the shortcut pass scans a candidate:
 *   n_pts = (int)fl(dist / check_step) + 2 points of extend_path's linspace, a point in collision iff mpb_collision_check
 *   says so (chained fields included), the scan stops after the 64 points that hold the first hit.  a == b checks that point.
 *   flag: MPB_PRM_EDGE_FREE, first -1; MPB_PRM_EDGE_BLOCKED, first the index of the first point in collision;
 *   MPB_PRM_EDGE_BAD_INDEX: a or b outside 0 .. P-1 (never dereferenced), first -1; MPB_PRM_EDGE_TOO_LONG:
 *   fl(dist / check_step) not below 2^20 - 1 (a NaN included), first -1.
 *   Refusals, in this order: E < 0, P < 1 or D < 1: MPB_E_INVALID; D > MPB_MAX_DOF: MPB_E_UNSUPPORTED; check_step not
 *   finite or <= 0; a null pointer; geom not 16-byte aligned: MPB_E_INVALID.  E == 0: MPB_OK, nothing launched.
 *
 * mpb_prm_query: the roadmap as data -- nodes (M,D), nbr (M,K) int32, w (M,K) fp32 -- and per query starts, goals (Q,D), the
 *   connection tables cs, cg (Q,Kc) int32 with ws, wg (Q,Kc) fp32, and direct (Q) fp32 -> paths (Q,Lmax,D), lengths (Q)
 *   int32, costs (Q) fp32, status (Q) int32.  No geometry is read.  A table entry is FINITE when its weight's bits are below
 *   +inf's (0 <= w < +inf, sign clear) and its index lies in 0 .. M-1; every other entry is absent (the caller writes +inf for
 *   an edge that is not FREE or is shorter than MPB_PRM_MIN_EDGE: such nodes are duplicates for planning).
 *   The graph is undirected: each finite entry (i, nbr[i][k], w[i][k]) relaxes both ways.  d is the least fixed point of
 *   d[v] = min(init[v], min_u fl(d[u] + w_uv)), init[v] the smallest finite ws entry that names v (+inf: none); sweeps run
 *   until one changes nothing (at most M).  fl(+) is monotone, so the fixed point -- the same bits on every run -- does not
 *   depend on the order of the relaxations.  The goal's cost is c = min_k fl(d[cg_k] + wg_k) over the finite entries, ties to
 *   the smallest k; the path is walked back from that cg_k after convergence, from d alone: the predecessor of v is the start
 *   when init[v] == d[v], else the smallest-index neighbour u with fl(d[u] + w_uv) == d[v] and d[u] < d[v] (d falls strictly
 *   along the walk: it cannot loop).  paths: start, the nodes, goal; rows at and past the length are zeros.
 *   status: MPB_PRM_OK; MPB_PRM_NO_START / MPB_PRM_NO_GOAL: no finite ws / wg entry; MPB_PRM_DISCONNECTED: no finite c;
 *   MPB_PRM_PATH_TOO_LONG: the path has more than Lmax rows; MPB_PRM_DEGENERATE: a node of the walk has no predecessor
 *   (weights so small against d that fl(d + w) == d).  Every status but OK: lengths 0, costs +inf, a zeroed path.
 *   A finite direct[q] (the start-goal distance where that segment is free, else +inf) wins before anything else: the path
 *   [start, goal], cost direct, MPB_PRM_OK.
 *   Refusals, in this order: Q < 0 or D < 1: MPB_E_INVALID; D > MPB_MAX_DOF, M > MPB_PRM_MAX_NODES, K or Kc >
 *   MPB_PRM_MAX_K: MPB_E_UNSUPPORTED; M < 2; K < 1 or Kc < 1; Lmax outside 2 .. MPB_PRM_MAX_PATH_ROWS; a null pointer:
 *   MPB_E_INVALID.  Q == 0: MPB_OK, nothing launched.
 * ------------------------------------------------------------------------------------------- */
#define MPB_PRM_MAX_NODES 16384
#define MPB_PRM_MAX_K 32
#define MPB_PRM_MAX_PATH_ROWS 1048576
#define MPB_PRM_MIN_EDGE 1e-4f
#define MPB_PRM_EDGE_FREE 0
#define MPB_PRM_EDGE_BLOCKED 1
#define MPB_PRM_EDGE_BAD_INDEX 2
#define MPB_PRM_EDGE_TOO_LONG 3
#define MPB_PRM_OK 0
#define MPB_PRM_NO_START 1
#define MPB_PRM_NO_GOAL 2
#define MPB_PRM_DISCONNECTED 3
#define MPB_PRM_PATH_TOO_LONG 4
#define MPB_PRM_DEGENERATE 5
int mpb_prm_knn(const float *queries, const float *nodes, int *idx, float *dist, int Q, int M, int D, int K,
                int exclude_self, void *stream);
int mpb_prm_edge_check(const float *pts, const int *pairs, int *flag, int *first, const float *geom, int geom_flags,
                       int P, int E, int D, float check_step, void *stream);
int mpb_prm_query(const float *nodes, const int *nbr, const float *w, const float *starts, const float *goals,
                  const int *cs, const float *ws, const int *cg, const float *wg, const float *direct, float *paths,
                  int *lengths, float *costs, int *status, int Q, int M, int K, int Kc, int D, int Lmax, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Time parameterisation of a trajectory batch under per-joint velocity and acceleration limits (the reference has no retiming:
 * build-defined): the time-optimal rest-to-rest timing along each path by reachability-based path
 * parameterisation (TOPP-RA, Pham & Pham 2018), for limits symmetric about zero.  Two launches: the timing, then the trajectory
 * sampled at a fixed control period.  No atomics: the same bits on every run.  Every operation below is rounded to fp32 on its
 * own (no fma).
 *
 * mpb_traj_retime: trajs: N trajectories of H rows, read in place as mpb_traj_collision_stats reads them (row h of trajectory n
 *   starts at trajs + (n*H + h)*row_stride, its first D floats are the joint positions q_h, the other columns are never read).
 *   v_max, a_max (D) device fp32, finite and > 0; sdot_max > 0 caps the path speed where the path does not move.
 *   Path parameter: the waypoint index.  Unknowns x_i = sdot^2 at the waypoints, u_i = sddot constant on [i, i+1]:
 *   x_{i+1} = x_i + 2 u_i; rest to rest, x_0 = x_{H-1} = 0.
 *   Path derivatives: p_i = (q_{i+1} - q_{i-1}) * 0.5, c_i = (q_{i+1} - q_i) - (q_i - q_{i-1}); p_0 = q_1 - q_0, p_{H-1} = q_{H-1} -
 *   q_{H-2}, c_0 = c_{H-1} = 0.
 *   Lines of interval i, each a u + b x <= c, in 2D + 1 pairs (a, b, c+, c-) that stand for a u + b x <= c+ and -a u - b x <= c-:
 *     joint j at waypoint i:      (p_ij, c_ij, a_j, a_j);
 *     joint j at waypoint i + 1:  (p_{i+1,j} + 2 c_{i+1,j}, c_{i+1,j}, a_j, a_j)       (the limit there, written in x_i);
 *     reachability:               (2, 1, beta_{i+1}, 0)                                 (0 <= x_{i+1} <= beta_{i+1}).
 *   Of a pair with a != 0 the line with a positive coefficient of u bounds u from above, the other from below; a pair with a == 0 and
 *   b != 0 bounds x by c+ / |b|.
 *   Speed limit: xv_i = min(sdot_max, min_j v_j / |p_ij| over p_ij != 0)^2.
 *   Backward: beta_{H-1} = 0; for i = H-2 .. 1, beta_i = the minimum of xv_i, of the x-only bounds, and over every (upper line 1, lower
 *   line 2) with k = a1 b2 - a2 b1 > 0 of (a1 c2 - a2 c1) / k.  (A minimum is exact in any order; (u, x) = (0, 0) satisfies every
 *   line: there is no infeasible case.)
 *   Forward: x_0 = 0; for i = 0 .. H-2, u_i = the minimum over the upper lines of (c - b x_i) / a, x_{i+1} = max(0, min(beta_{i+1},
 *   x_i + 2 u_i)).  Times: t_0 = 0, t_{i+1} = t_i + 2 / (sqrt(x_i) + sqrt(x_{i+1})) (exact for constant sddot).
 *   Outputs: x (N,H), u (N,H-1), t (N,H), qd (N,H,D) = p_i sqrt(x_i), status (N) int32: MPB_RETIME_OK, or MPB_RETIME_STALLED when two
 *   adjacent x are 0 or t_{H-1} is not finite or exceeds t_max (repeated waypoints do this: the caller purges them); x, u, t, qd
 *   are written as computed (t is +inf from the stall on).  A v_max / a_max entry that is not finite and > 0: STALLED, all four
 *   outputs zero.
 *   GUARANTEE: the limits hold at the waypoints (the acceleration at both ends of every interval), to rounding.  Between the
 *   waypoints they do not: the answer to an overstep there is a denser input (mpb_traj_interpolate) or scaled limits.
 *   Refusals, in this order, all before the first HIP call: D > MPB_MAX_DOF; H > MPB_MAX_H: MPB_E_UNSUPPORTED; H < 3, N < 0, D < 1
 *   or row_stride < D; sdot_max, then t_max, not finite or <= 0; a null pointer: MPB_E_INVALID.  N == 0: MPB_OK, nothing launched.
 *
 * mpb_traj_retime_sample: trajs as above, x, u, t, retime_status as mpb_traj_retime wrote them -> out (N,T_rows,2D): row k of
 *   trajectory n is the state (positions, velocities) at tau = fl32(k * dt); n_rows (N) int32, status (N) int32.  With T = t_{H-1}:
 *   tau < T: i the interval with t_i <= tau < t_{i+1}, d = tau - t_i, r = sqrt(x_i), sigma = clamp(r d + ((u_i d) d) * 0.5, 0, 1),
 *     sdot = max(0, r + u_i d); with dq = q_{i+1} - q_i, e2 = (3 dq - 2 p_i) - p_{i+1}, e3 = (p_i + p_{i+1}) - 2 dq -- the cubic Hermite of
 *     (q_i, p_i, q_{i+1}, p_{i+1}) -- position q_i + sigma (p_i + sigma (e2 + sigma e3)), velocity (p_i + sigma (2 e2 + (3 sigma) e3))
 *     sdot.
 *   tau >= T: the last waypoint, zero velocity (the batch is padded by holding).
 *   n_rows = ceil(T / dt) + 1, the quotient of the two fp32 values taken in fp64 (beyond an int: INT_MAX); n_rows > T_rows:
 *   MPB_RETIME_TOO_LONG, the T_rows rows that fit are still written.  retime_status != MPB_RETIME_OK or T not finite:
 *   MPB_RETIME_STALLED, n_rows = 0, every row holds the first waypoint with zero velocity.
 *   Refusals, in this order, all before the first HIP call: D > MPB_MAX_DOF; H > MPB_MAX_H: MPB_E_UNSUPPORTED; H < 3, N < 0, D < 1
 *   or row_stride < D; dt not finite or <= 0; T_rows < 1; N * ceil(T_rows / 256) beyond an int; a null pointer: MPB_E_INVALID.
 *   N == 0: MPB_OK, nothing launched.
 * ------------------------------------------------------------------------------------------- */
#define MPB_RETIME_OK 0
#define MPB_RETIME_STALLED 1
#define MPB_RETIME_TOO_LONG 2
int mpb_traj_retime(const float *trajs, size_t row_stride, const float *v_max, const float *a_max, float *x, float *u,
                    float *t, float *qd, int *status, int N, int H, int D, float sdot_max, float t_max, void *stream);
int mpb_traj_retime_sample(const float *trajs, size_t row_stride, const float *x, const float *u, const float *t,
                           const int *retime_status, float *out, int *n_rows, int *status, int N, int H, int D, float dt,
                           int T_rows, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Linear segments with parabolic blends: a joint-space polyline turned into a trajectory a controller can run (Kunz & Stilman 2012,
 * the idea behind MoveIt's TOTG; the reference has none: build-defined, DESIGN.md 10 has the proofs).  Constant velocity along
 * every segment, a constant-acceleration blend around every waypoint, a cap on how far a blend may leave its corner.  The limits
 * hold for EVERY t (not at samples), the trajectory is C1 and rest to rest, and every point of it lies within a known per-joint
 * distance of a point of the polyline.  It is NOT time-optimal.  Two launches: the timing, then the trajectory sampled at a fixed
 * control period.  No atomics: the same bits on every run.  Every operation below is rounded to fp32 on its own (no fma).
 *
 * mpb_path_blend: paths: N paths of H rows read in place as mpb_traj_retime reads them (row h of path n starts at
 *   paths + (n*H + h)*row_stride, its first D floats are the joint positions q_h); lengths (N) int32 or NULL (every path has H rows):
 *   path n is the polyline through its rows 0 .. L-1, 2 <= L <= H, the rows past them are never read.  v_max, a_max (D) device fp32,
 *   finite and > 0; max_deviation = delta > 0, a joint-space infinity-norm in rad, +inf: no cap; max_sweeps >= 1
 *   (MPB_BLEND_DEFAULT_MAX_SWEEPS).
 *   Segments i = 0 .. L-2, waypoints i = 0 .. L-1, dq_i = q_{i+1} - q_i, T_i = max_k (|dq_ik| / v_k) to start with.  Then, repeated:
 *     v_i = dq_i / T_i, v_{-1} = v_{L-1} = 0;  dv_i = v_i - v_{i-1};  tb_i = max_k (|dv_ik| / a_k);  mdv_i = max_k |dv_ik|;
 *     cap_i = (8 delta) / mdv_i, none where mdv_i == 0 or delta = +inf;  m_i = min(T_{i-1}, T_i, cap_i) over those that exist.
 *     Waypoint i is in violation iff tb_i > m_i.  No waypoint in violation: done.  Otherwise, when max_sweeps rescalings have been
 *     made: MPB_BLEND_NOT_CONVERGED; else f_i = sqrt(m_i / tb_i) at the waypoints in violation and 1 elsewhere, and
 *     T_i <- T_i / min(f_i, f_{i+1}) for every segment: one more rescaling (slowing both segments of a waypoint by f scales its tb by
 *     f and its T and cap by 1 / f).
 *   Then tw_0 = tb_0 * 0.5, tw_{i+1} = tw_i + T_i summed in this order, duration = tw_{L-1} + tb_{L-1} * 0.5,
 *   dev_i = (mdv_i * tb_i) * 0.125 = max_k |dv_ik| tb_i / 8: inside the blend of waypoint i joint k is never farther than
 *   |dv_ik| tb_i / 8 <= delta from the polyline; tb_i <= min(T_{i-1}, T_i): neighbouring blends do not overlap.
 *   Outputs: T (N,H-1), tb, tw, dev (N,H), duration (N), sweeps (N) int32 the rescalings made, status (N) int32, first_bad (N) int32.
 *   MPB_BLEND_DEGENERATE_SEGMENT: a segment with max_k |dq_ik| == 0 (the caller purges duplicates), first_bad its index (the lowest);
 *   MPB_BLEND_BAD_INPUT: a length outside 2 .. H, a non-finite coordinate in the path's rows, a limit that is not finite and > 0;
 *   first_bad is -1 except for a DEGENERATE_SEGMENT.  A path that is not MPB_BLEND_OK has zeros in T, tb, tw, dev and duration 0;
 *   an OK path has zeros at and past its length.
 *   Refusals, in this order, all before the first HIP call: D > MPB_MAX_DOF; H > MPB_MAX_H: MPB_E_UNSUPPORTED; H < 2, N < 0, D < 1
 *   or row_stride < D; max_deviation not > 0 or NaN; max_sweeps < 1; a null pointer (lengths may be NULL): MPB_E_INVALID.
 *   N == 0: MPB_OK, nothing launched.
 *
 * mpb_path_blend_sample: paths, lengths as above, T, tb, tw, duration, blend_status as mpb_path_blend wrote them -> out (N,T_rows,3D):
 *   row k of path n is the state (positions, velocities, accelerations) at tau = fl32(k * dt); n_rows (N) int32, status (N) int32.
 *   With a_i = dv_i / tb_i, 0 where tb_i == 0 (v, dv formed from the rows and T as above):
 *   tau >= duration: the last waypoint at rest.  Else j the last waypoint with tw_j <= tau (none: the window of waypoint 0; j = L-1:
 *     its window); tau is in the window of j when tau - tw_j <= tb_j * 0.5, else in that of j + 1 when tw_{j+1} - tau <= tb_{j+1} * 0.5,
 *     else on segment j.  In the window of waypoint i, d = tau - tw_i, s = d + tb_i * 0.5:
 *       q = (q_i + v_{i-1} d) + ((a_i s) s) * 0.5,  qd = v_{i-1} + a_i s,  qdd = a_i;
 *     on segment j, d = tau - tw_j:  q = q_j + v_j d,  qd = v_j,  qdd = 0.
 *   Row 0 is q_0 at rest exactly (s = 0, v_{-1} = 0).
 *   n_rows = ceil(duration / dt) + 1, the quotient of the two fp32 values taken in fp64 (beyond an int: INT_MAX); n_rows > T_rows:
 *   MPB_BLEND_TOO_LONG, the T_rows rows that fit are still written.  blend_status != MPB_BLEND_OK: that status, n_rows = 0, every row
 *   holds the first waypoint at rest (so does a length outside 2 .. H or a duration that is not finite: MPB_BLEND_BAD_INPUT).
 *   Refusals, in this order, all before the first HIP call: D > MPB_MAX_DOF; H > MPB_MAX_H: MPB_E_UNSUPPORTED; H < 2, N < 0, D < 1
 *   or row_stride < D; dt not finite or <= 0; T_rows < 1; N * ceil(T_rows / 256) beyond an int; a null pointer (lengths may be
 *   NULL): MPB_E_INVALID.  N == 0: MPB_OK, nothing launched.
 * ------------------------------------------------------------------------------------------- */
int mpb_path_blend(const float *paths, size_t row_stride, const int *lengths, const float *v_max, const float *a_max,
                   float max_deviation, int max_sweeps, float *T, float *tb, float *tw, float *dev, float *duration, int *sweeps,
                   int *status, int *first_bad, int N, int H, int D, void *stream);
int mpb_path_blend_sample(const float *paths, size_t row_stride, const int *lengths, const float *T, const float *tb,
                          const float *tw, const float *duration, const int *blend_status, float *out, int *n_rows, int *status,
                          int N, int H, int D, float dt, int T_rows, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Clearance, and the certificate that a joint-space polyline is free BETWEEN its samples (build-defined; definition, proof and
 * what is not built: DESIGN.md 10).  Obstacle geometry only: spheres and axis-aligned boxes, chained fields included.
 *   eta_l(q) = min_f (sd_f(x_l(q)) - margin_f) - r_l,   eta(q) = min_l eta_l(q)
 * sd_f the exact signed distance of field f (the minimum over its obstacles, walked exhaustively: the broad-phase grids only know
 * obstacles within the margin), x_l the collision-sphere centres, r_l their radii; fscale plays no part.  eta_l < 0 is the
 * predicate of mpb_collision_check.  Every chained field must carry the robot's WHOLE link table (pack_geometry with
 * prune_static=False): the walk reads the first field's.
 *
 * mpb_clearance: q (N, D) -> eta (N) and link (N) int, the arg-min sphere (lowest index on a tie; may be NULL).  One lane per
 *   configuration.  A geometry header that does not hold D joints: eta = NaN, link = -1.
 *   Refusals: D > MPB_MAX_DOF: MPB_E_UNSUPPORTED; N < 0, D < 1: MPB_E_INVALID; (N == 0: MPB_OK;) a null q / geom / eta, geom not
 *   16-byte aligned: MPB_E_INVALID.
 *
 * mpb_path_certify: N paths of H rows read in place as mpb_traj_collision_stats reads them (row h of path n starts at
 *   paths + (n*H + h)*row_stride, its first D floats are read); lengths (N) or NULL (every path has H rows); path n is the polyline
 *   through its first lengths[n] rows.  reach: the device buffer of MPB_REACH_HEADER_WORDS header words (MPB_REACH_MAGIC, n_dof,
 *   n_links, kind) and rho as [n_dof][n_links] floats -- sphere l is never farther than rho_il from the origin of joint i when joint
 *   i moves it, 0 when it does not (certify_layout.reach_table builds it in fp64, rounded up); n_links: its sphere count.
 *   On the segment a -> b sphere l moves at most w * Lambda_l while the parameter moves by w, Lambda_l = sum_i |b_i - a_i| rho_il
 *   (a point robot: |b - a|_2); the device multiplies its fp32 sum by MPB_CERT_LAMBDA_INFLATE.
 *   Level -1: every node; eta - c_req < -S at a node: MPB_CERT_COLLISION, witness (node index, t = 0).  Then level d = 0, 1, ...:
 *   the intervals of a level in (segment, j) order, interval j of segment s at level d has the midpoint parameter
 *   t = (2j + 1) 2^-(d+1), the half-width w = 2^-(d+1) and the midpoint m = fmaf(b - a, t, a) per joint, and is
 *     FREE       when eta_l(m) - w Lambda_l - c_req > S for every l  (then eta_l - c_req > S on the closed interval),
 *     COLLISION  when eta_l(m) - c_req < -S for some l,
 *     else split into (2j, 2j + 1) at level d + 1; at d == max_depth it stays undecided.
 *   A path ends at the first level that holds a COLLISION interval (witness: the smallest (segment, t) of that level, the arg-min
 *   sphere and its eta); else MPB_CERT_UNDECIDED_QUEUE when the next level would hold more than max_intervals intervals (level 0:
 *   more than max_intervals segments), nothing further being evaluated; else MPB_CERT_UNDECIDED_DEPTH when an interval of level
 *   max_depth stayed undecided, else MPB_CERT_FREE.  MPB_CERT_BAD_INPUT: a length outside 1 .. H or a non-finite coordinate;
 *   MPB_CERT_BUFFER_CHANGED: a geometry or reach header that differs from (D, n_links) -- nothing else of either buffer is read.
 *   out_i (N, MPB_CERT_OUT_INTS): status, witness segment, witness link, n_evals (configurations evaluated), depth_max (the deepest
 *   level evaluated, -1: nodes only); out_f (N, MPB_CERT_OUT_FLOATS): witness t, witness eta, margin_cert -- the minimum over the
 *   FREE intervals of eta_l - w Lambda_l - c_req (a path of one row: its node's eta - c_req), a lower bound of the path's clearance
 *   minus c_req up to S; -inf unless the status is MPB_CERT_FREE.  Without a witness: segment = link = -1, t = eta = 0.
 *   One single-wave workgroup per path, the level's queue in LDS, no atomics, every loop bounded: the same bits on every run.
 *   Refusals, in this order, all before the launch: D > MPB_MAX_DOF: MPB_E_UNSUPPORTED; H outside 1 .. MPB_CERT_MAX_ROWS (the
 *   segment field of the interval word), max_depth outside 0 .. MPB_CERT_MAX_DEPTH (its j field), max_intervals outside
 *   1 .. MPB_CERT_MAX_INTERVALS, n_links outside 1 .. MPB_CERT_MAX_LINKS: MPB_E_UNSUPPORTED, each by name; N < 0, D < 1,
 *   row_stride < D, S not finite or negative, c_req not finite: MPB_E_INVALID; (N == 0: MPB_OK;) a null required pointer, geom or
 *   reach not 16-byte aligned: MPB_E_INVALID.
 * ------------------------------------------------------------------------------------------- */
int mpb_clearance(const float *q, const float *geom, float *eta, int *link, int N, int D, void *stream);
int mpb_path_certify(const float *paths, size_t row_stride, const int *lengths, const float *geom, const float *reach, int n_links,
                     float S, float c_req, int max_depth, int max_intervals, int *out_i, float *out_f, int N, int H, int D,
                     void *stream);

/* ---------------------------------------------------------------------------------------------
 * The world: ONE in-kernel collision predicate over a whole planning task (build-defined).  A configuration is in
 * collision iff  c_obs(q) > 0  or  c_sdf(q) > 0  or  c_self(q) > 0,  where c_obs is mpb_collision_check's gap on geom, c_sdf is
 * mpb_sdf_grid_collision_check's gap on the packed SDF-grid buffer sdfb, c_self is mpb_self_collision_check's gap on the packed self
 * buffer selfb: the answer of the three stand-alone predicates ORed, in one launch and inside the kernels that decide collisions in
 * a loop.  sdfb and selfb are device buffers as those predicates take them (validated on the host by mpb_sdf_grid_check /
 * mpb_self_check; their headers are read once per address, mpb_sdf_grid_invalidate / mpb_self_invalidate announce another buffer at
 * an address); EITHER MAY BE NULL: that part is absent.  With both null every entry below launches its old entry's kernels and gives
 * its outputs bit for bit (mpb_world_collision_check: mpb_collision_check's flags, and its gap as part 0).
 * A buffer whose header no longer holds what the launcher read puts every configuration in collision (the stand-alone predicates'
 * rule; its part reads NaN, a validation max_gap 3e38): an RRT problem then ends START_OR_GOAL_IN_COLLISION, a shortcut candidate is
 * REJECTed at point 0; no status word is added and nothing is read through a header word the launcher has not checked.
 * Every *_world entry takes its old entry's arguments plus (sdfb, selfb) after geom_flags, makes the old entry's refusals first, in the
 * old order and under its own name, then: sdfb or selfb not 16-byte aligned: MPB_E_INVALID; the SDF header's refusals
 * (mpb_sdf_grid_check's, of the header), its n_dof != D: MPB_E_INVALID; the self header's refusals, its n_dof != D: MPB_E_INVALID.
 * LDS: the self part keeps 768 B per collision sphere and wave next to what the old kernel takes (mpb_path_shortcut_world refuses
 * an Lmax whose path does not fit beside it).
 *
 * mpb_world_collision_check: q (N, D); in_collision (N) bytes, 0 / 1; parts (N, 3) optional (may be NULL): (c_obs, c_sdf, c_self), an
 *   absent part 0 -- the bits of the three stand-alone gaps.  Refusals as mpb_collision_check's, then the above.
 * mpb_rrt_connect_init_world / mpb_rrt_connect_run_world: mpb_rrt_connect_init / _run with the world predicate for the start / goal
 *   check and for every point of an extension.  Workspace layout, magic and status values are those of mpb_rrt_connect_*; a
 *   workspace may be initialised and advanced by either pair of entries as long as one world is used throughout.  (The world kernels
 *   are instantiated for the compile-time Panda and for run-time D: the bits of a D = 2, 3, 7 tree on a world are those of the
 *   run-time-D kernel, which rounds the nearest-node distance as rrt_connect_kernel<0, 0> does.)
 * mpb_path_shortcut_world: mpb_path_shortcut with the world predicate on a candidate's points.
 * mpb_traj_collision_stats_world: mpb_traj_collision_stats with the world predicate on the dense points; max_gap is the largest
 *   (c_obs + c_sdf) + c_self, every addition rounded.  Workgroups of 256 threads, of 64 where selfb is given (one self block).
 * ------------------------------------------------------------------------------------------- */
int mpb_world_collision_check(const float *q, const float *geom, int geom_flags, const float *sdfb, const float *selfb,
                              unsigned char *in_collision, float *parts, int N, int D, void *stream);
int mpb_rrt_connect_init_world(void *workspace, size_t workspace_bytes, const float *start, const float *goal, const float *geom,
                               int geom_flags, const float *sdfb, const float *selfb, int B, int max_nodes, int n_pre, int D,
                               void *stream);
int mpb_rrt_connect_run_world(void *workspace, size_t workspace_bytes, const float *geom, int geom_flags, const float *sdfb,
                              const float *selfb, const float *pre_samples, size_t pre_stride, const int *sample_idx, float *paths,
                              int *lengths, int *status, int B, int max_nodes, int n_pre, int D, int Lmax, int iter0, int n_iters,
                              int total_iters, float step_size, float n_radius, uint64_t seed, uint32_t problem_offset, void *stream);
int mpb_path_shortcut_world(const float *paths_in, const int *lengths_in, float *paths_out, int *lengths_out, float *stats, int *log,
                            const float *geom, int geom_flags, const float *sdfb, const float *selfb, const float *draws, int N,
                            int Lmax, int D, int n_iters, float check_step, uint64_t seed, uint32_t problem_offset, void *stream);
int mpb_traj_collision_stats_world(const float *trajs, size_t row_stride, const float *geom, int geom_flags, const float *sdfb,
                                   const float *selfb, int n_interp, int *n_in_collision, int *first_in_collision, float *max_gap,
                                   unsigned char *point_in_collision, int N, int H, int D, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Clearance of a timed trajectory against a moving-obstacle field, and the certificate that it is free over the whole CONTINUUM of its
 * clock, between the rows too (build-defined; definition, proof and what is not built: DESIGN.md 10).  Every other entry that sees a
 * moving-obstacle buffer decides collisions at the rows only.
 * The continuum.  A trajectory of R rows and the packed moving-obstacle buffer of the same R rows (mpb_moving_check's format): for
 * segment h = 0 .. R - 2 and s in [0, 1] the robot stands at q(h, s) = q_h + s (q_{h+1} - q_h) and moving obstacle o (spheres first,
 * then boxes) has its centre on the CHORD c_o(h, s) = c_{o,h} + s (c_{o,h+1} - c_{o,h}) of the buffer's own per-row centres; boxes
 * translate and do not rotate.  The static scene is the geometry chain `geom`, as in mpb_path_certify.
 *   eta_l(h, s) = min( eta_static_l(q),  min_o sd_o(x_l(q); c_o(h, s)) - (margin_moving + r_l) ),     eta = min_l eta_l
 * eta_static_l is mpb_clearance's eta_l, bit for bit; margin_moving is the buffer's header word.  At a node (s = 0) the sign of the
 * moving part is mpb_moving_collision_check's answer for that row up to ties within the slack (thr = margin + r_l rounded once as there).
 * Motion bound.  sphere_sd and box_sd are 1-Lipschitz in the query point AND in the centre.  Over a parameter half-width w about a
 * midpoint the pair (robot sphere l, moving obstacle o) changes its distance by at most w (Lambda_l + V_{o,h}): Lambda_l the reach sum
 * of mpb_path_certify (the same reach buffer, the same MPB_CERT_LAMBDA_INFLATE), V_{o,h} = |c_{o,h+1} - c_{o,h}| formed per lane in
 * fp32 from the two rows' centres and inflated the same way; a static pair by w Lambda_l.
 *
 * mpb_moving_clearance: trajs of N x R rows read in place (row h of trajectory n starts at trajs + (n*R + h)*row_stride, its first D
 *   floats are read); eta (N, R), link (N, R) the arg-min robot sphere (lowest index on a tie) and obstacle (N, R) the arg-min
 *   obstacle of every row AT ITS OWN TIME: o >= 0 a moving obstacle, -1 - f the static field f of the chain (a tie between the two:
 *   the static scene).  link and obstacle may be NULL.  One lane per (trajectory, row).  A geometry or moving header that differs
 *   from what the launcher read: eta = NaN, link = -1, obstacle = MPB_STC_NO_OBSTACLE.
 *   Refusals, in this order: D > MPB_MAX_DOF, R outside 1 .. MPB_MOVING_MAX_ROWS: MPB_E_UNSUPPORTED; N < 0, D < 1, row_stride < D:
 *   MPB_E_INVALID; (N == 0: MPB_OK;) a null trajs / geom / moving / eta, geom or moving not 16-byte aligned: MPB_E_INVALID; the
 *   moving header's refusals (read once per address: mpb_moving_invalidate), its n_dof != D, its n_rows != R: MPB_E_INVALID.
 *
 * mpb_traj_certify_moving: the bisection of mpb_path_certify on that continuum.  Level -1: every node against its own row's centres;
 *   eta - c_req < -S: MPB_CERT_COLLISION, witness (row, s = 0).  Level d = 0, 1, ...: interval j of segment h has the midpoint
 *   parameter s = (2j + 1) 2^-(d+1), the half-width w = 2^-(d+1), the robot at fmaf(q_{h+1} - q_h, s, q_h) and obstacle o at
 *   fmaf(c_{o,h+1} - c_{o,h}, s, c_{o,h}) per coordinate, and is
 *     FREE       when min over pairs of (eta_pair - w bound_pair) - c_req > S  (then eta - c_req > S on the closed interval),
 *     COLLISION  when eta - c_req < -S at the midpoint,
 *     else split; the queue order, max_depth, max_intervals and the statuses are mpb_path_certify's, unchanged in meaning
 *   (MPB_CERT_BAD_INPUT: a non-finite coordinate; MPB_CERT_BUFFER_CHANGED: a geometry, moving or reach header that differs from what
 *   the launcher read -- nothing else of the buffers is read).
 *   out_i (N, MPB_STC_OUT_INTS): status, witness row h, witness link, witness obstacle (o >= 0 moving, -1 - f static field f),
 *   n_evals, depth_max; out_f (N, MPB_STC_OUT_FLOATS): witness s, witness eta, margin_cert (-inf unless MPB_CERT_FREE).  Without a
 *   witness: row = link = -1, obstacle = MPB_STC_NO_OBSTACLE, s = eta = 0.  The witness TIME t_start + (h + s) dt_row is the
 *   caller's to form (in fp64: the buffer carries no clock).  MPB_STC_NOT_VALID is never written by the kernel: it is what a caller
 *   gives a trajectory it did not submit.
 *   The certificate is about the CHORD motion of the buffer's centres.  Where the field's own motion has a keyframe strictly inside
 *   a row interval the caller raises c_req by the largest deviation of the two (st_certify_layout.chord_deviation, host, fp64).
 *   One single-wave workgroup per trajectory, the level's queue in LDS, no atomics, every loop bounded: the same bits on every run.
 *   Refusals, in this order, all before the launch: D > MPB_MAX_DOF, R outside 1 .. MPB_MOVING_MAX_ROWS, max_depth outside
 *   0 .. MPB_CERT_MAX_DEPTH, max_intervals outside 1 .. MPB_CERT_MAX_INTERVALS, n_links outside 1 .. MPB_MOVING_MAX_LINKS:
 *   MPB_E_UNSUPPORTED, each by name; N < 0, D < 1, row_stride < D, S not finite or negative, c_req not finite: MPB_E_INVALID;
 *   (N == 0: MPB_OK;) a null required pointer, geom / moving / reach not 16-byte aligned: MPB_E_INVALID; the moving header's
 *   refusals, its n_dof != D, its n_rows != R, its n_links != n_links: MPB_E_INVALID.
 * ------------------------------------------------------------------------------------------- */
int mpb_moving_clearance(const float *trajs, size_t row_stride, const float *geom, const float *moving, float *eta, int *link,
                         int *obstacle, int N, int R, int D, void *stream);
int mpb_traj_certify_moving(const float *trajs, size_t row_stride, const float *geom, const float *moving, const float *reach,
                            int n_links, float S, float c_req, int max_depth, int max_intervals, int *out_i, float *out_f, int N,
                            int R, int D, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MPB_H */

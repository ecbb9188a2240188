// mpb_rrt_star.hip -- batched RRT* and informed RRT* (rrt_star.py:133-261 over rrt_base.py:59-63, :94-119 and
// utils.py:4-50).
//
// ONE persistent launch runs up to n_iters loop bodies for B independent problems, one single-wave workgroup per problem,
// resumable from the caller's workspace in chunks like mpb_rrt_connect_run.  Workgroups never wait on each other, there is
// no spin wait, and every loop is bounded by n_iters, max_nodes, the pool length, the point count of one extension or the
// node count (retrace, relaxation sweeps, candidate walk).  The body restates the reference's line by line:
//   - the two stopping rules at the top, in the reference's order, on counters carried in the workspace header;
//   - goal or sample draw (:185), informed rejection (:197-199), nearest node, extend_path, safe_path, the deletion of a
//     reached pool entry (:210-211), the append with d and cost, goal detection (:216);
//   - neighbours within n_radius (:225-231, n_knn == 0) and the rewire walk (:243-251) in two phases.  Costs only decrease
//     while the reference walks the neighbours, so the neighbours that pass `new.cost + d < n.cost` against the costs at
//     the START of the walk are a superset of those that pass at their turn.  Phase 1 (parallel) finds those candidates,
//     keeps them in ascending index order in the workspace, and checks their edges new -> n with the (candidate, point)
//     pairs flattened over the 64 lanes.  Phase 2 (sequential, index order) re-tests each candidate against the CURRENT
//     cost, rewires, and propagates costs before the next candidate is tested;
//   - cost propagation: the reference keeps cost[i] == fl32(cost[parent[i]] + d[i]) at all times (root: 0); given parents
//     and d that fixed point is unique, so relaxation sweeps over all nodes, repeated until a ballot reports no change
//     (at most node-count sweeps), reproduce the reference's bits although parent < child no longer holds.
// ONE distance routine (rrt_dist of mpb_rrt.h) serves nearest node, extension, neighbours, rewire, goal and informed tests: a distance
// between the same two bit patterns is the same number wherever it is computed, which is what resolves the reference's
// exact ties (new.cost + d == n.cost when the new node duplicates its parent) the way the reference does.
#include "mpb_rrt.h"
#include "mpb_rrt_host.h"

#define RRS_WORDS_PER_NODE 18.0  // the size bound of rrt_shape_check: the padded row, parent, d, cost, three of scratch
#define RRS_NO_BEST 3.0e38f      // best_cost_eps before the first success (the reference's torch.inf)

struct RrsLayout {
    size_t hdr, goalq, nodes, parents, d, cost, cand, pool, total;   // offsets in 32-bit words
    int Dp, pool_words;
};

__host__ __device__ static inline RrsLayout rrs_layout(int B, int max_nodes, int n_pre, int D) {
    RrsLayout L;
    L.Dp = (D + 3) & ~3;
    L.pool_words = (n_pre + 1) / 2;
    L.hdr = MPB_RRT_GLOBAL_WORDS;
    L.goalq = L.hdr + (size_t)B * MPB_RRT_STAR_HDR_WORDS;
    L.nodes = L.goalq + (size_t)B * L.Dp;
    L.parents = L.nodes + (size_t)B * max_nodes * L.Dp;
    L.d = L.parents + (size_t)B * max_nodes;
    L.cost = L.d + (size_t)B * max_nodes;
    L.cand = L.cost + (size_t)B * max_nodes;                          // candidate index, d, edge verdict: 3 x max_nodes
    L.pool = L.cand + (size_t)B * 3 * max_nodes;
    L.total = L.pool + (size_t)B * L.pool_words;
    return L;
}

// ---- workspace initialisation: root, goal, counters, pool list, start / goal collision check -------------------------
template <int MODEL>
__global__ __launch_bounds__(64) void rrs_init_kernel(int* __restrict__ ws, const float* __restrict__ start,
                                                      const float* __restrict__ goal, const float* __restrict__ geom, int B,
                                                      int max_nodes, int n_pre, int D) {
    __shared__ unsigned gridw[MPB_GRID_MAX_CELLS];
    __shared__ float4 otab[MPB_GRID_MAX_SPH + 1];
    const int b = blockIdx.x, lane = threadIdx.x;
    const RrsLayout L = rrs_layout(B, max_nodes, n_pre, D);
    unsigned* pool = reinterpret_cast<unsigned*>(ws) + L.pool + (size_t)b * L.pool_words;
    const int status = rrt_init_shared<MODEL>(ws, MPB_RRT_STAR_MAGIC, B, max_nodes, n_pre, D, L.Dp, pool, L.pool_words, start, goal, geom,
                                              gridw, otab, b, lane);
    float* wf = reinterpret_cast<float*>(ws);
    if (lane < L.Dp) {
        wf[L.nodes + (size_t)b * max_nodes * L.Dp + lane] = (lane < D) ? start[(size_t)b * D + lane] : 0.f;
        wf[L.goalq + (size_t)b * L.Dp + lane] = (lane < D) ? goal[(size_t)b * D + lane] : 0.f;
    }
    if (lane == 0) {
        ws[L.parents + (size_t)b * max_nodes] = -1;
        wf[L.d + (size_t)b * max_nodes] = 0.f;
        wf[L.cost + (size_t)b * max_nodes] = 0.f;
    }
    if (lane < MPB_RRT_STAR_HDR_WORDS) {
        int v = 0;
        if (lane == MPB_RRTS_STATUS) v = status;
        if (lane == MPB_RRTS_COUNT) v = 1;
        if (lane == MPB_RRTS_GOAL || lane == MPB_RRTS_FIRST_ITER) v = -1;
        if (lane == MPB_RRTS_POOL_LEN) v = n_pre;
        if (lane == MPB_RRTS_BEST_COST_EPS) v = __float_as_int(RRS_NO_BEST);
        ws[L.hdr + (size_t)b * MPB_RRT_STAR_HDR_WORDS + lane] = v;
    }
}

struct RrsArgs {
    int* ws;
    const float* geom;
    const float* pre;
    size_t pre_stride;
    const int* sample_idx;
    const int* goal_draw;
    float* paths;
    int* lengths;
    float* costs;
    int* status;
    int B, D, max_nodes, n_pre, Lmax, iter0, n_iters, total_iters, max_bci, n_after, informed;
    float step, radius, goal_prob, cost_eps, eps;
    uint32_t seed_lo, seed_hi, problem_offset;
};

// ---- the persistent kernel ------------------------------------------------------------------------------------------
template <int DT, int MODEL>
__global__ __launch_bounds__(64) void rrt_star_kernel(const RrsArgs a) {
#pragma clang fp contract(off)
    __shared__ unsigned gridw[MPB_GRID_MAX_CELLS];
    __shared__ float4 otab[MPB_GRID_MAX_SPH + 1];
    __shared__ unsigned short pool[MPB_RRT_MAX_PRE_SAMPLES];
    __shared__ int s_excl[64], s_first[64];
    constexpr int DM = DT ? DT : MPB_MAX_DOF;
    const int D = DT ? DT : a.D;
    const int b = blockIdx.x, lane = threadIdx.x;
    const RrsLayout L = rrs_layout(a.B, a.max_nodes, a.n_pre, D);
    int* H = a.ws + L.hdr + (size_t)b * MPB_RRT_STAR_HDR_WORDS;
    int status = H[MPB_RRTS_STATUS];
    if (status != MPB_RRT_RUNNING) {                       // block-uniform: a finished problem costs nothing
        if (lane == 0) a.status[b] = status;
        return;
    }
    int it = H[MPB_RRTS_ITERS], cnt = H[MPB_RRTS_COUNT], goal = H[MPB_RRTS_GOAL], plen = H[MPB_RRTS_POOL_LEN];
    int stop = MPB_RRT_STOP_RUNNING, bci = H[MPB_RRTS_BEST_COST_ITERS], iafs = H[MPB_RRTS_ITERS_AFTER_FIRST_SUCCESS];
    int rewires = H[MPB_RRTS_REWIRES], rejected = H[MPB_RRTS_INFORMED_REJECTIONS];
    float best = __int_as_float(H[MPB_RRTS_BEST_COST_EPS]);
    float* wf = reinterpret_cast<float*>(a.ws);
    float* nodes_b = wf + L.nodes + (size_t)b * a.max_nodes * L.Dp;
    int* parents_b = a.ws + L.parents + (size_t)b * a.max_nodes;
    float* d_b = wf + L.d + (size_t)b * a.max_nodes;
    float* cost_b = wf + L.cost + (size_t)b * a.max_nodes;
    int* cand_i = a.ws + L.cand + (size_t)b * 3 * a.max_nodes;
    float* cand_d = reinterpret_cast<float*>(cand_i + a.max_nodes);
    int* cand_ok = cand_i + 2 * (size_t)a.max_nodes;
    unsigned short* pool_g = reinterpret_cast<unsigned short*>(a.ws + L.pool + (size_t)b * L.pool_words);
    for (int i = lane; i < plen; i += 64) pool[i] = pool_g[i];
    const float* pre_b = a.pre + (size_t)b * a.pre_stride;
    float* path_b = a.paths + (size_t)b * a.Lmax * D;
    const float* staged = nullptr;
    float sq[MPB_MAX_DOF], gq[MPB_MAX_DOF];
    rrt_load_row4<DM>(nodes_b, L.Dp, sq);
    rrt_load_row4<DM>(wf + L.goalq + (size_t)b * L.Dp, L.Dp, gq);
    __syncthreads();

    const int it_end = min(a.iter0 + a.n_iters, a.total_iters);
    for (; it < it_end && status == MPB_RRT_RUNNING; ++it) {
        // ---- :167-182: the stopping rules, in the reference's order
        if (bci >= a.max_bci) { stop = MPB_RRT_STOP_COST_CONVERGED; ++it; break; }
        if (goal >= 0) {
            const float gc = cost_b[goal];
            if (gc < best - a.cost_eps) { best = gc; bci = 0; }
            else ++bci;
            ++iafs;
        }
        if (a.n_after >= 0 && iafs > a.n_after) { stop = MPB_RRT_STOP_AFTER_SUCCESS; ++it; break; }
        // ---- :185-189: goal or sample
        bool do_goal;
        int idx;
        if (a.sample_idx != nullptr) {
            do_goal = goal < 0 && (it == 0 || a.goal_draw[(size_t)b * a.total_iters + it] != 0);
            idx = a.sample_idx[(size_t)b * a.total_iters + it];
            idx = min(max(idx, 0), max(plen - 1, 0));
        } else {
            const uint4 r = philox4x32_10(make_uint4(a.problem_offset + (uint32_t)b, (uint32_t)it, MPB_RRT_STAR_MAGIC, 0u),
                                          make_uint2(a.seed_lo, a.seed_hi));
            idx = (int)__umulhi(r.x, (uint32_t)plen);
            do_goal = goal < 0 && (it == 0 || (float)(r.y >> 8) * (1.0f / 16777216.0f) < a.goal_prob);
        }
        float tq[MPB_MAX_DOF];
        if (do_goal) {
#pragma unroll
            for (int k = 0; k < MPB_MAX_DOF; ++k) tq[k] = gq[k];
        } else {
            if (plen == 0) { status = MPB_RRT_POOL_EMPTY; break; }
            const float* trow = pre_b + (size_t)pool[idx] * D;
#pragma unroll
            for (int k = 0; k < MPB_MAX_DOF; ++k) tq[k] = (k < DM && k < D) ? trow[k] : 0.f;
        }
        // ---- :197-199: informed rejection (a goal node exists, so this was a sample draw)
        if (a.informed && goal >= 0) {
            if (rrt_dist<DM>(sq, tq) + rrt_dist<DM>(tq, gq) >= cost_b[goal]) {
                rrt_pool_delete(pool, idx, plen, lane);
                --plen;
                ++rejected;
                continue;
            }
        }
        // ---- :202: nearest node (the lowest index wins a tie, as torch.argmin does).  (The other pieces of mpb_rrt.h are spelled out in
        // this kernel: called here they cost SGPR spills in the run-time-D form or 1.5 % of the time -- DESIGN.md, the RRT open items.)
        float bestd = 3.0e38f;
        int bi = 0x7FFFFFFF;
        for (int i = lane; i < cnt; i += 64) {
            float r[MPB_MAX_DOF];
            rrt_load_row4<DM>(nodes_b + (size_t)i * L.Dp, L.Dp, r);
            const float ds = rrt_dist<DM>(r, tq);
            if (ds < bestd) { bestd = ds; bi = i; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float od = __shfl_xor(bestd, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (od < bestd || (od == bestd && oi < bi)) { bestd = od; bi = oi; }
        }
        // ---- :205-208: extend_path (the far end clamped to n_radius, the point count from the UNCLAMPED distance), safe_path
        const float dist = bestd;
        float q1[MPB_MAX_DOF], dl[MPB_MAX_DOF], nq[MPB_MAX_DOF];
        rrt_load_row4<DM>(nodes_b + (size_t)bi * L.Dp, L.Dp, q1);
        // (max_dist / dist with a Python float on the left is Tensor.__rtruediv__: dist.reciprocal() * max_dist, two roundings)
        const float f = (dist > a.radius) ? (1.0f / dist) * a.radius : 1.0f;
#pragma unroll
        for (int k = 0; k < MPB_MAX_DOF; ++k) {
            const float df = tq[k] - q1[k];
            const float q2 = (dist > a.radius) ? fmaf(df, f, q1[k]) : tq[k];
            dl[k] = q2 - q1[k];
        }
        const int n_pts = rrt_point_count(dist, a.step);
        const float lstep = 1.0f / (float)(n_pts - 1);
        const int first = rrt_first_collision<DM, MODEL>(a.geom, gridw, otab, staged, q1, dl, n_pts, lstep, lane);
        if (first == 0) continue;
        rrt_linspace_point<DM>(q1, dl, n_pts, lstep, first < 0 ? n_pts - 1 : first - 1, nq);
        // ---- :210-211: a reached sample leaves the pool
        if (!do_goal) {
            bool reached = true;
#pragma unroll
            for (int k = 0; k < MPB_MAX_DOF; ++k)
                if (k < DM && k < D) reached = reached && rrt_close(nq[k], tq[k]);
            if (reached) {
                rrt_pool_delete(pool, idx, plen, lane);
                --plen;
            }
        }
        // ---- :213-222: the new node (d == 0 when the first free point is the nearest node itself: a duplicate)
        const int n = cnt;
        if (n >= a.max_nodes) { status = MPB_RRT_TREE_FULL; break; }
        const float dn = rrt_dist<DM>(q1, nq);
        const float cn = cost_b[bi] + dn;
        {
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < DM; ++k) v = (lane == k) ? nq[k] : v;
            if (lane < L.Dp) nodes_b[(size_t)n * L.Dp + lane] = v;
            if (lane == 0) { parents_b[n] = bi; d_b[n] = dn; cost_b[n] = cn; }
        }
        if (do_goal && rrt_dist<DM>(nq, gq) < a.eps) {       // :216
            goal = n;
            if (lane == 0) {
                H[MPB_RRTS_FIRST_COST] = __float_as_int(cn); H[MPB_RRTS_FIRST_ITER] = it; H[MPB_RRTS_FIRST_COUNT] = n + 1;
            }
        }
        cnt = n + 1;
        __syncthreads();
        // ---- :225-251 phase 1a: the neighbours (distance < n_radius) that pass the rewire test against the costs as they are now
        int ncand = 0;
        for (int base = 0; base < cnt; base += 64) {
            const int i = base + lane;
            float r[MPB_MAX_DOF];
            rrt_load_row4<DM>(nodes_b + (size_t)min(i, cnt - 1) * L.Dp, L.Dp, r);
            const float di = rrt_dist<DM>(r, nq);
            const bool c = i < cnt && di < a.radius && cn + di < cost_b[min(i, cnt - 1)];
            const unsigned long long m = __ballot(c);
            if (c) {
                const int pos = ncand + __popcll(m & ((1ull << lane) - 1ull));
                cand_i[pos] = i;
                cand_d[pos] = di;
            }
            ncand += __popcll(m);
        }
        if (ncand == 0) continue;
        __syncthreads();
        // ---- phase 1b: the candidates' edges new -> n (extend_path + safe_path, :246-250), (candidate, point) pairs over the lanes
        for (int cb = 0; cb < ncand; cb += 64) {
            const int c = cb + lane;
            const bool cv = c < ncand;
            const int ci = cand_i[min(c, ncand - 1)];
            const float cd = cand_d[min(c, ncand - 1)];
            const int np = cv ? rrt_point_count(cd, a.step) : 0;
            int inc = np;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int t = __shfl_up(inc, off, 64);
                if (lane >= off) inc += t;
            }
            const int total = __shfl(inc, 63, 64);
            s_excl[lane] = inc - np;
            s_first[lane] = 0x7FFFFFFF;
            __syncthreads();
            for (int fb = 0; fb < total; fb += 64) {
                const int fl = min(fb + lane, total - 1);
                int j = 0;
#pragma unroll
                for (int s = 32; s > 0; s >>= 1)
                    if (s_excl[j + s] <= fl) j += s;
                const int p = fl - s_excl[j];
                const int cj = min(cb + j, ncand - 1);
                float tj[MPB_MAX_DOF], dj[MPB_MAX_DOF], q[MPB_MAX_DOF];
                rrt_load_row4<DM>(nodes_b + (size_t)cand_i[cj] * L.Dp, L.Dp, tj);
#pragma unroll
                for (int k = 0; k < MPB_MAX_DOF; ++k) dj[k] = tj[k] - nq[k];
                const int npj = rrt_point_count(cand_d[cj], a.step);
                rrt_linspace_point<DM>(nq, dj, npj, 1.0f / (float)(npj - 1), min(p, npj - 1), q);
                const float cc = rrt_config_cost<MODEL>(a.geom, gridw, otab, staged, q);
                if (fb + lane < total && cc > 0.f) atomicMin(&s_first[j], p);
            }
            __syncthreads();
            // the verdict of candidate c: the edge's last free point lies within eps of n (:249-250)
            const int fc = s_first[lane];
            bool ok = false;
            if (cv && fc != 0) {
                float tj[MPB_MAX_DOF], dj[MPB_MAX_DOF], q[MPB_MAX_DOF];
                rrt_load_row4<DM>(nodes_b + (size_t)ci * L.Dp, L.Dp, tj);
#pragma unroll
                for (int k = 0; k < MPB_MAX_DOF; ++k) dj[k] = tj[k] - nq[k];
                rrt_linspace_point<DM>(nq, dj, np, 1.0f / (float)(np - 1), fc == 0x7FFFFFFF ? np - 1 : fc - 1, q);
                ok = rrt_dist<DM>(tj, q) < a.eps;
            }
            if (cv) cand_ok[c] = ok ? 1 : 0;
            __syncthreads();
        }
        // ---- phase 2: index order, against the CURRENT costs; propagation finishes before the next candidate is tested
        for (int c = 0; c < ncand; ++c) {
            if (cand_ok[c] == 0) continue;
            const int ci = cand_i[c];
            const float cd = cand_d[c];
            if (!(cn + cd < cost_b[ci])) continue;
            __syncthreads();
            if (lane == 0) { parents_b[ci] = n; d_b[ci] = cd; }
            ++rewires;
            __syncthreads();
            for (int sweep = 0; sweep < cnt; ++sweep) {
                bool changed = false;
                for (int base = 1; base < cnt; base += 64) {
                    const int i = base + lane;
                    if (i < cnt) {
                        const float want = cost_b[parents_b[i]] + d_b[i];
                        if (want != cost_b[i]) { cost_b[i] = want; changed = true; }
                    }
                    __syncthreads();
                }
                if (__ballot(changed) == 0ull) break;
            }
        }
    }
    if (status == MPB_RRT_RUNNING && stop == MPB_RRT_STOP_RUNNING && it >= a.total_iters) stop = MPB_RRT_STOP_ITERS;
    if (status == MPB_RRT_TREE_FULL && goal >= 0) stop = MPB_RRT_STOP_TREE_FULL;
    if (status == MPB_RRT_POOL_EMPTY && goal >= 0) stop = MPB_RRT_STOP_POOL_EMPTY;
    if (stop != MPB_RRT_STOP_RUNNING) status = (goal >= 0) ? MPB_RRT_FOUND : MPB_RRT_EXHAUSTED_ITERS;
    __syncthreads();
    // ---- every launch leaves the current best path behind: retrace root -> goal (:259), purge_duplicates_from_traj (:261)
    if (goal >= 0) {
        int len = 0;
        for (int j = goal; j >= 0 && len < cnt; j = parents_b[j]) ++len;
        if (len > a.Lmax) {
            status = MPB_RRT_PATH_TOO_LONG;
            if (lane == 0) a.lengths[b] = 0;
        } else {
            int pos = len - 1;
            for (int j = goal; j >= 0 && pos >= 0; j = parents_b[j], --pos)
                if (lane < D) path_b[(size_t)pos * D + lane] = nodes_b[(size_t)j * L.Dp + lane];
            __syncthreads();
            const int kept = rrt_purge(path_b, len, D, lane);
            if (lane == 0) { a.lengths[b] = kept; a.costs[b] = cost_b[goal]; }
        }
    }
    for (int i = lane; i < plen; i += 64) pool_g[i] = pool[i];
    if (lane == 0) {
        H[MPB_RRTS_STATUS] = status; H[MPB_RRTS_ITERS] = it; H[MPB_RRTS_COUNT] = cnt; H[MPB_RRTS_GOAL] = goal;
        H[MPB_RRTS_POOL_LEN] = plen; H[MPB_RRTS_STOP_REASON] = stop; H[MPB_RRTS_BEST_COST_ITERS] = bci;
        H[MPB_RRTS_ITERS_AFTER_FIRST_SUCCESS] = iafs; H[MPB_RRTS_BEST_COST_EPS] = __float_as_int(best);
        H[MPB_RRTS_REWIRES] = rewires; H[MPB_RRTS_INFORMED_REJECTIONS] = rejected;
        a.status[b] = status;
    }
}

// ---- host side (the checks: mpb_rrt_host.h) -------------------------------------------------------------------------
extern "C" size_t mpb_rrt_star_workspace_bytes(int B, int max_nodes, int n_pre, int D) {
    if (rrt_shape_check("mpb_rrt_star_workspace_bytes", RRS_WORDS_PER_NODE, B, max_nodes, n_pre, D) != MPB_OK) return 0;
    return 4 * rrs_layout(B, max_nodes, n_pre, D).total;
}

extern "C" int mpb_rrt_star_init(void* workspace, size_t workspace_bytes, const float* start, const float* goal,
                                 const float* geom, int geom_flags, int B, int max_nodes, int n_pre, int D, void* stream) {
    const int rc = rrt_init_check("mpb_rrt_star_init", RRS_WORDS_PER_NODE, B, max_nodes, n_pre, D, !workspace || !start || !goal || !geom, false,
                                  workspace, geom, workspace_bytes, 4 * rrs_layout(B, max_nodes, n_pre, D).total);
    if (rc != MPB_OK || B == 0) return rc;
    if (rrt_use_model(geom_flags, D))
        hipLaunchKernelGGL(rrs_init_kernel<PandaModel::ID>, dim3(B), dim3(64), 0, (hipStream_t)stream, (int*)workspace, start, goal, geom, B, max_nodes, n_pre, D);
    else
        hipLaunchKernelGGL(rrs_init_kernel<0>, dim3(B), dim3(64), 0, (hipStream_t)stream, (int*)workspace, start, goal, geom, B, max_nodes, n_pre, D);
    return mpb_check_launch("mpb_rrt_star_init");
}

extern "C" int mpb_rrt_star_run(void* workspace, size_t workspace_bytes, const float* geom, int geom_flags,
                                const float* pre_samples, size_t pre_stride, const int* sample_idx, const int* goal_draw,
                                float* paths, int* lengths, float* costs, int* status, int B, int max_nodes, int n_pre, int D,
                                int Lmax, int iter0, int n_iters, int total_iters, int max_best_cost_iters,
                                int n_iters_after_success, int informed, float step_size, float n_radius, float goal_prob,
                                float cost_eps, float eps, uint64_t seed, uint32_t problem_offset, void* stream) {
    int rc = rrt_init_check("mpb_rrt_star_run", RRS_WORDS_PER_NODE, B, max_nodes, n_pre, D, !workspace || !geom || !pre_samples || !paths || !lengths || !costs || !status,
                            (sample_idx == nullptr) != (goal_draw == nullptr), workspace, geom, workspace_bytes, 4 * rrs_layout(B, max_nodes, n_pre, D).total);
    if (rc == MPB_OK) rc = rrt_run_check("mpb_rrt_star_run", Lmax, iter0, n_iters, total_iters, max_best_cost_iters >= 0, step_size, n_radius);
    if (rc != MPB_OK || B == 0) return rc;
    const RrsArgs a = {(int*)workspace, geom, pre_samples, pre_stride, sample_idx, goal_draw, paths, lengths, costs, status,
                       B, D, max_nodes, n_pre, Lmax, iter0, n_iters, total_iters, max_best_cost_iters, n_iters_after_success,
                       informed, step_size, n_radius, goal_prob, cost_eps, eps, (uint32_t)seed, (uint32_t)(seed >> 32), problem_offset};
    return rrt_dispatch<2, 7>(geom_flags, D, [&](auto dt, auto model) {      // (no form of its own for D = 3)
        hipLaunchKernelGGL((rrt_star_kernel<dt.value, model.value>), dim3(B), dim3(64), 0, (hipStream_t)stream, a);
        return mpb_check_launch("mpb_rrt_star_run");
    });
}

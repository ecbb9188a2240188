// mpb_rrt_connect_loop.h -- the body of the persistent RRT-Connect kernel: the TEXT of rrt_connect_kernel<DT, MODEL> and of its world form
// rrtc_world_kernel<DT, MODEL> (mpb_rrt_connect.hip), included inside each with RRT_WORLD defined (0 / 1), `a` the kernel's RrtArgs and
// `W` a const WorldView* (null with RRT_WORLD == 0).  It is text and not a function because the compiler lays the wrapped form out
// differently (other VGPR and SGPR-spill counts in every instantiation), and the figures and bits of the five plain
// instantiations are pinned (tests/test_path_shortcut_cpu.py, tests/test_gpu_sample_based_bits.py).  No include guard: included twice.
#pragma clang fp contract(off)
    __shared__ unsigned gridw[MPB_GRID_MAX_CELLS];
    __shared__ float4 otab[MPB_GRID_MAX_SPH + 1];
    __shared__ unsigned short pool[MPB_RRT_MAX_PRE_SAMPLES];
    constexpr int DM = DT ? DT : MPB_MAX_DOF;
    const int D = DT ? DT : a.D;
    const int b = blockIdx.x, lane = threadIdx.x;
    const RrtLayout L = rrt_layout(a.B, a.max_nodes, a.n_pre, D);
    int* H = a.ws + L.hdr + (size_t)b * MPB_RRT_CONNECT_HDR_WORDS;
    int status = H[MPB_RRTC_STATUS];
    if (status != MPB_RRT_RUNNING) {                       // block-uniform: a finished problem costs nothing
        if (lane == 0) a.status[b] = status;
        return;
    }
    int cnt[2] = {H[MPB_RRTC_COUNTS], H[MPB_RRTC_COUNTS + 1]};
    int bit = H[MPB_RRTC_SWAP], plen = H[MPB_RRTC_POOL_LEN];
    float* nodes_b = reinterpret_cast<float*>(a.ws) + L.nodes + (size_t)b * 2 * a.max_nodes * L.Dp;
    int* parents_b = a.ws + L.parents + (size_t)b * 2 * a.max_nodes;
    unsigned short* pool_g = reinterpret_cast<unsigned short*>(a.ws + L.pool + (size_t)b * L.pool_words);
    for (int i = lane; i < plen; i += 64) pool[i] = pool_g[i];
    const float* pre_b = a.pre + (size_t)b * a.pre_stride;
    float* path_b = a.paths + (size_t)b * a.Lmax * D;
    const float* staged = nullptr;
    __syncthreads();

    // one extension (extend_path + safe_path + the append): grows tree t from its node nearest to `tq` towards `tq`;
    // returns false when the extension's first point is in collision (safe_path's []) or the tree is full
    float nq[MPB_MAX_DOF];
    auto extend = [&](int t, const float (&tq)[MPB_MAX_DOF]) -> bool {
        const float* nd = nodes_b + (size_t)t * a.max_nodes * L.Dp;
        const int n = cnt[t];
        float best = 3.0e38f;
        int bi = 0x7FFFFFFF;
        for (int i = lane; i < n; i += 64) {
            const float ds = sqrtf(rrtc_row_d2<DM>(nd + (size_t)i * L.Dp, L.Dp, tq));
            if (ds < best) { best = ds; bi = i; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float od = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (od < best || (od == best && oi < bi)) { best = od; bi = oi; }
        }
        const float dist = best;
        float q1[MPB_MAX_DOF], dl[MPB_MAX_DOF];
        const float f = (dist > a.radius) ? a.radius / dist : 1.0f;
#pragma unroll
        for (int k = 0; k < MPB_MAX_DOF; ++k) {
            q1[k] = (k < DM && k < D) ? nd[(size_t)bi * L.Dp + k] : 0.f;
            const float df = tq[k] - q1[k];
            // (utils.py:7-8: the far end clamped to n_radius; the point count below is from the UNCLAMPED distance)
            const float q2 = (dist > a.radius) ? fmaf(df, f, q1[k]) : tq[k];
            dl[k] = q2 - q1[k];
        }
        const int n_pts = rrt_point_count(dist, a.step);
        const float lstep = 1.0f / (float)(n_pts - 1);
        const int first = rrt_first_collision<DM, MODEL, RRT_WORLD>(a.geom, gridw, otab, staged, q1, dl, n_pts, lstep, lane, W);
        if (first == 0) return false;
        rrt_linspace_point<DM>(q1, dl, n_pts, lstep, first < 0 ? n_pts - 1 : first - 1, nq);
        if (n >= a.max_nodes) {
            status = MPB_RRT_TREE_FULL;
            return false;
        }
        float* dst = nodes_b + ((size_t)t * a.max_nodes + n) * L.Dp;
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < DM; ++k) v = (lane == k) ? nq[k] : v;
        if (lane < L.Dp) dst[lane] = v;
        if (lane == 0) parents_b[(size_t)t * a.max_nodes + n] = bi;
        cnt[t] = n + 1;
        __syncthreads();                                   // the node is read back by the next nearest-node scan
        return true;
    };

    int it = a.iter0;
    const int it_end = min(a.iter0 + a.n_iters, a.total_iters);
    for (; it < it_end && status == MPB_RRT_RUNNING; ++it) {
        if (plen == 0) { status = MPB_RRT_POOL_EMPTY; break; }
        bit ^= 1;                                          // rrt_connect.py:126-128
        const int t1 = bit, t2 = bit ^ 1;
        int idx;
        if (a.sample_idx != nullptr) {
            idx = a.sample_idx[(size_t)b * a.total_iters + it];
            idx = min(max(idx, 0), plen - 1);
        } else {
            const uint4 r = philox4x32_10(make_uint4(a.problem_offset + (uint32_t)b, (uint32_t)it, MPB_RRT_CONNECT_MAGIC, 0u),
                                          make_uint2(a.seed_lo, a.seed_hi));
            idx = (int)__umulhi(r.x, (uint32_t)plen);
        }
        const float* trow = pre_b + (size_t)pool[idx] * D;
        float tq[MPB_MAX_DOF];
#pragma unroll
        for (int k = 0; k < MPB_MAX_DOF; ++k) tq[k] = (k < DM && k < D) ? trow[k] : 0.f;
        if (!extend(t1, tq)) continue;                     // :142-143 -- BEFORE the swap-back (Q15)
        float n1[MPB_MAX_DOF];
        bool reached = true;
#pragma unroll
        for (int k = 0; k < MPB_MAX_DOF; ++k) {
            n1[k] = nq[k];
            if (k < DM && k < D) reached = reached && rrt_close(n1[k], tq[k]);
        }
        if (reached) {                                     // :149-150, rrt_base.py:59-63: delete entry idx, keep the order
            rrt_pool_delete(pool, idx, plen, lane);
            --plen;
        }
        if (!extend(t2, n1)) continue;                     // :161-162
        bit ^= 1;                                          // :168-170
        bool joined = true;
#pragma unroll
        for (int k = 0; k < MPB_MAX_DOF; ++k)
            if (k < DM && k < D) joined = joined && rrt_close(n1[k], nq[k]);
        if (!joined) continue;
        // ---- :173-185: retrace(n2)[:-1] + reversed(retrace(n1)), then purge_duplicates_from_traj (utils.py:33-50)
        const float* ndA = nodes_b + (size_t)t2 * a.max_nodes * L.Dp;
        const float* ndB = nodes_b + (size_t)t1 * a.max_nodes * L.Dp;
        const int* paA = parents_b + (size_t)t2 * a.max_nodes;
        const int* paB = parents_b + (size_t)t1 * a.max_nodes;
        int lenA = 0, lenB = 0;
        for (int j = paA[cnt[t2] - 1]; j >= 0 && lenA < cnt[t2]; j = paA[j]) ++lenA;
        for (int j = cnt[t1] - 1; j >= 0 && lenB < cnt[t1]; j = paB[j]) ++lenB;
        const int Lraw = lenA + lenB;
        ++it;
        if (Lraw > a.Lmax) { status = MPB_RRT_PATH_TOO_LONG; break; }
        {
            int pos = lenA - 1;
            for (int j = paA[cnt[t2] - 1]; j >= 0 && pos >= 0; j = paA[j], --pos)
                if (lane < D) path_b[(size_t)pos * D + lane] = ndA[(size_t)j * L.Dp + lane];
            pos = lenA;
            for (int j = cnt[t1] - 1; j >= 0 && pos < Lraw; j = paB[j], ++pos)
                if (lane < D) path_b[(size_t)pos * D + lane] = ndB[(size_t)j * L.Dp + lane];
        }
        __syncthreads();
        const int len = rrt_purge(path_b, Lraw, D, lane);
        if (lane == 0) a.lengths[b] = len;
        status = MPB_RRT_FOUND;
        break;
    }
    if (status == MPB_RRT_RUNNING && it >= a.total_iters) status = MPB_RRT_EXHAUSTED_ITERS;
    __syncthreads();
    for (int i = lane; i < plen; i += 64) pool_g[i] = pool[i];
    if (lane == 0) {
        H[MPB_RRTC_STATUS] = status; H[MPB_RRTC_ITERS] = it; H[MPB_RRTC_COUNTS] = cnt[0]; H[MPB_RRTC_COUNTS + 1] = cnt[1];
        H[MPB_RRTC_SWAP] = bit; H[MPB_RRTC_POOL_LEN] = plen;
        a.status[b] = status;
    }

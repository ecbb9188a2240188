// mpb_lib.hip -- what belongs to the whole library rather than to one planner: the last-error buffer, mpb_version /
// mpb_last_error, and the host-side validator of a packed geometry buffer (mpb_geom_check, mpb_geom_flags).  No kernel.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "mpb_common.h"
#include "mpb_host.h"
#include "mpb_geom.h"

static thread_local char g_err[512] = "";
char* mpb_err_buf() { return g_err; }

#ifdef MPB_TUNING_BUILD
extern "C" int mpb_version(void) { return MPB_ABI_VERSION | MPB_VERSION_TUNING_BUILD; }
#else
extern "C" int mpb_version(void) { return MPB_ABI_VERSION; }
#endif
extern "C" const char* mpb_last_error(void) { return g_err; }

// A buffer tagged with a compile-time robot model (header word `model`) must carry exactly that model's tables: the joint
// transforms bit for bit, and as link table the model's collision spheres selected by the keep mask (word `keep_mask`), of
// which only spheres on frame 1 may be missing.  The model kernels never read these tables -- they trust the tag.
template <class M>
static int model_check_as(const float* g, const char* who) {
    const int32_t* gi = reinterpret_cast<const int32_t*>(g);
    const uint32_t keep = (uint32_t)gi[MPB_GW_KEEP_MASK];
    if (gi[MPB_GW_KIND] != MPB_KIND_CHAIN || gi[MPB_GW_N_DOF] != M::N_DOF || gi[MPB_GW_N_TF] != M::N_TF) return mpb_failf(MPB_E_INVALID, "%s: model tag does not match the robot", who);
    if (memcmp(g + gi[MPB_GW_OFF_TF], M::TF, sizeof(float) * 12 * M::N_TF) != 0) return mpb_failf(MPB_E_INVALID, "%s: joint transforms differ from the tagged model", who);
    int n = 0;
    for (int l = 0; l < M::N_LINKS; ++l) {
        if (!((keep >> l) & 1u)) {
            if (M::LINK_FRAME[l] != 1) return mpb_failf(MPB_E_INVALID, "%s: only frame-1 spheres of a model may be pruned", who);
            continue;
        }
        if (n >= gi[MPB_GW_N_LINKS]) return mpb_failf(MPB_E_INVALID, "%s: keep mask and link table disagree", who);
        const float* lk = g + gi[MPB_GW_OFF_LINKS] + 8 * n;
        if (reinterpret_cast<const int32_t*>(lk)[0] != M::LINK_FRAME[l] || memcmp(lk + 1, M::LINK[l], 4 * sizeof(float)) != 0)
            return mpb_failf(MPB_E_INVALID, "%s: link table differs from the tagged model", who);
        ++n;
    }
    if (n != gi[MPB_GW_N_LINKS] || (M::N_LINKS < 32 && (keep >> M::N_LINKS) != 0u)) return mpb_failf(MPB_E_INVALID, "%s: keep mask and link table disagree", who);
    // the model kernels clamp a hinge to [0, 1] (mpb_geom.h, UNIT): margin + largest collision sphere + deepest possible
    // penetration (sphere radius / smallest half extent of a box) must stay below 1
    float rl_max = 0.f, deepest = 0.f;
    for (int l = 0; l < M::N_LINKS; ++l) rl_max = M::LINK[l][3] > rl_max ? M::LINK[l][3] : rl_max;
    for (int o = 0; o < gi[MPB_GW_N_SPH]; ++o) deepest = g[gi[MPB_GW_OFF_SPH] + 4 * o + 3] > deepest ? g[gi[MPB_GW_OFF_SPH] + 4 * o + 3] : deepest;
    for (int o = 0; o < gi[MPB_GW_N_BOX]; ++o) {
        const float* h = g + gi[MPB_GW_OFF_BOX] + 8 * o + 4;
        const float m = h[0] < h[1] ? (h[0] < h[2] ? h[0] : h[2]) : (h[1] < h[2] ? h[1] : h[2]);
        deepest = m > deepest ? m : deepest;
    }
    if (!(g[MPB_GW_MARGIN] + rl_max + deepest < 1.0f)) return mpb_failf(MPB_E_INVALID, "%s: a model-tagged scene must keep every hinge below 1 (margin + radii)", who);
    return MPB_OK;
}

static int model_check(const float* g, const char* who) {
    const int model = reinterpret_cast<const int32_t*>(g)[MPB_GW_MODEL];
    if (model == 0) return MPB_OK;
    if (model == PandaModel::ID) return model_check_as<PandaModel>(g, who);
    return mpb_failf(MPB_E_INVALID, "%s: unknown robot model id", who);
}

static int geom_check_one(const float* g, int n_words, const char* who) {
    if (!g || n_words < MPB_GEOM_HEADER_WORDS) return mpb_failf(MPB_E_INVALID, "%s: geometry buffer too small", who);
    const int32_t* gi = reinterpret_cast<const int32_t*>(g);
    if (gi[MPB_GW_MAGIC] != MPB_GEOM_MAGIC || (gi[MPB_GW_VERSION] != MPB_GEOM_VERSION && gi[MPB_GW_VERSION] != MPB_GEOM_VERSION_LIST)) return mpb_failf(MPB_E_INVALID, "%s: bad magic/version", who);
    const bool list = gi[MPB_GW_VERSION] == MPB_GEOM_VERSION_LIST;       // version 7: the grid section is a list grid (mpb_geom.h, spheres_hinge_list)
    const int kind = gi[MPB_GW_KIND], n_dof = gi[MPB_GW_N_DOF], n_tf = gi[MPB_GW_N_TF], n_links = gi[MPB_GW_N_LINKS], n_sph = gi[MPB_GW_N_SPH], n_box = gi[MPB_GW_N_BOX];
    if (kind != MPB_KIND_POINT && kind != MPB_KIND_CHAIN) return mpb_failf(MPB_E_INVALID, "%s: unknown robot kind", who);
    if (n_dof < 1 || n_dof > MPB_MAX_DOF) return mpb_failf(MPB_E_INVALID, "%s: n_dof out of range", who);
    if (kind == MPB_KIND_POINT && (n_dof < 2 || n_dof > 3 || n_links != 1)) return mpb_failf(MPB_E_INVALID, "%s: point robot must be 2-D/3-D with one sphere", who);
    if (kind == MPB_KIND_CHAIN && n_tf != n_dof + 1) return mpb_failf(MPB_E_INVALID, "%s: chain needs n_dof+1 transforms", who);
    if (n_links < 1 || n_sph < 0 || n_box < 0 || n_sph + n_box < 1) return mpb_failf(MPB_E_INVALID, "%s: empty link/obstacle set", who);
    const int off_tf = gi[MPB_GW_OFF_TF], off_links = gi[MPB_GW_OFF_LINKS], off_sph = gi[MPB_GW_OFF_SPH], off_box = gi[MPB_GW_OFF_BOX], total = gi[MPB_GW_TOTAL];
    const int off_cull = gi[MPB_GW_OFF_CULL], off_fs = gi[MPB_GW_OFF_FS], off_grid = gi[MPB_GW_OFF_GRID];
    const int gnx = gi[MPB_GW_GRID_DIMS], gny = gi[MPB_GW_GRID_DIMS + 1], gnz = gi[MPB_GW_GRID_DIMS + 2], n_cells = gi[MPB_GW_N_CELLS];
    const int n_sph_pad = (n_sph + 3) / 4 * 4;
    const int n_frames = n_tf > 1 ? n_tf : 1;
    const int n_fs = (n_frames + 1 + 3) / 4 * 4;
    if (off_tf != MPB_GEOM_HEADER_WORDS || off_links != off_tf + 12 * n_tf || off_sph != off_links + 8 * n_links ||
        off_box != off_sph + 4 * n_sph || off_cull != off_box + 8 * n_box || off_fs != off_cull + 8 * n_sph_pad ||
        off_grid != off_fs + n_fs || total > n_words)
        return mpb_failf(MPB_E_INVALID, "%s: inconsistent section offsets", who);
    const int off_cand = off_grid + (n_cells + MPB_GRID_PAD - 1) / MPB_GRID_PAD * MPB_GRID_PAD;
    if (list ? (total < off_cand + 4 || ((total - off_cand) & 3)) : total != off_cand) return mpb_failf(MPB_E_INVALID, "%s: inconsistent section offsets", who);
    if (list && (n_cells < 1 || n_cells > MPB_GRID_MAX_CELLS || n_sph > MPB_LIST_MAX_SPH || n_box > MPB_LIST_MAX_BOX ||
                 4 * (total - off_cand) > MPB_LIST_MAX_CAND + 16))
        return mpb_failf(MPB_E_INVALID, "%s: a list grid needs 1..4096 cells, <= 255 spheres, <= 127 boxes, <= 16 KB of candidates", who);
    if ((off_links | off_sph | off_box | off_cull | off_fs | off_grid) & 3) return mpb_failf(MPB_E_INVALID, "%s: sections must be 16-byte aligned", who);
    if (n_cells < 0 || (n_cells > 0 && (gnx < 1 || gny < 1 || gnz < 1 || gnx * gny * gnz != n_cells)))
        return mpb_failf(MPB_E_INVALID, "%s: bad broad-phase grid dims", who);
    if (n_cells > 0) {
        // version 6: cells on a lattice through the origin -- lo = (K - 1/2) h per axis with integer K, and header word k_lin =
        // Kx + gnx (Ky + gny Kz): what grid_cell_rel (mpb_geom.h) turns round(x / h) into a cell with
        long K[3];
        for (int a = 0; a < 3; ++a) {
            if (!(g[MPB_GW_GRID_INV + a] > 0.f)) return mpb_failf(MPB_E_INVALID, "%s: bad grid cell size", who);
            const double k = (double)g[MPB_GW_GRID_LO + a] * (double)g[MPB_GW_GRID_INV + a] + 0.5;
            K[a] = lrint(k);
            // (lo and 1/h are fp32: their product carries ~|K| 1.2e-7 of rounding, so the tolerance scales with |K| -- an absolute
            // 1e-3 refused the grids build_grid makes beyond |K| ~ 16 700)
            if (fabs(k - (double)K[a]) > 1e-3 + 4e-7 * fabs((double)K[a]) || labs(K[a]) > 100000) return mpb_failf(MPB_E_INVALID, "%s: grid origin is not on the cell lattice", who);
        }
        if ((long)gi[MPB_GW_K_LIN] != K[0] + (long)gnx * (K[1] + (long)gny * K[2])) return mpb_failf(MPB_E_INVALID, "%s: grid lattice index (header word k_lin) does not match the origin", who);
        if (labs((long)gi[MPB_GW_K_LIN]) + (long)n_cells >= (1L << 21)) return mpb_failf(MPB_E_INVALID, "%s: grid too far from the origin for the fp32 cell index", who);
    }
    if (list) {   // every cell's candidate range must lie inside the candidate bytes and name existing obstacles
        const unsigned char* cand = reinterpret_cast<const unsigned char*>(g + off_cand);
        const int n_cand = 4 * (total - off_cand);
        for (int i = 0; i < n_cells; ++i) {
            const uint32_t w = (uint32_t)gi[off_grid + i];
            if (w & MPB_LIST_OVERFLOW) continue;                    // overflowing cell: the kernels test every obstacle
            const int start = (int)(w & MPB_LIST_START_MASK), ns = (int)((w >> MPB_LIST_NSPH_SHIFT) & MPB_LIST_NSPH_MASK),
                      nb = (int)((w >> MPB_LIST_NBOX_SHIFT) & MPB_LIST_NBOX_MASK);
            if ((w & MPB_LIST_RESERVED) || ns > MPB_LIST_CELL_MAX_SPH || nb > MPB_LIST_CELL_MAX_BOX || start + ns + nb > n_cand)
                return mpb_failf(MPB_E_INVALID, "%s: list-grid cell out of range", who);
            for (int k = 0; k < ns; ++k)
                if ((int)cand[start + k] >= n_sph) return mpb_failf(MPB_E_INVALID, "%s: grid cell references a missing obstacle", who);
            for (int k = 0; k < nb; ++k)
                if ((int)cand[start + ns + k] >= n_box) return mpb_failf(MPB_E_INVALID, "%s: grid cell references a missing obstacle", who);
        }
    } else
    for (int i = 0; i < n_cells; ++i) {   // every packed obstacle index must exist
        const uint32_t w = (uint32_t)gi[off_grid + i];
        if (w == MPB_GRID_OVERFLOW) continue;
        for (int k = 0; k < MPB_GRID_SLOTS; ++k) {
            const uint32_t idx = (w >> (MPB_GRID_SLOT_BITS * k)) & MPB_GRID_SLOT_MASK;      // n_sph = unused slot (the far dummy the kernels append)
            if ((int)idx > n_sph) return mpb_failf(MPB_E_INVALID, "%s: grid cell references a missing obstacle", who);
        }
    }
    // frame -> link ranges must be monotone and end at n_links
    for (int j = 0; j < n_frames; ++j)
        if (gi[off_fs + j] < 0 || gi[off_fs + j] > gi[off_fs + j + 1] || gi[off_fs + j + 1] > n_links)
            return mpb_failf(MPB_E_INVALID, "%s: bad frame_start table", who);
    if (gi[off_fs] != 0 || gi[off_fs + n_frames] != n_links) return mpb_failf(MPB_E_INVALID, "%s: frame_start must cover all links", who);
    int prev = 1;
    for (int l = 0; l < n_links; ++l) {
        const int f = gi[off_links + 8 * l];
        if (kind == MPB_KIND_CHAIN && (f < prev || f > n_dof + 1)) return mpb_failf(MPB_E_INVALID, "%s: link frames must be sorted in [1, n_dof+1]", who);
        prev = f > prev ? f : prev;
    }
    if (!(g[MPB_GW_FSCALE] >= 0.f)) return mpb_failf(MPB_E_INVALID, "%s: field scale must be >= 0", who);
    return model_check(g, who);
}


extern "C" int mpb_geom_check(const float* g, int n_words) {
    // a buffer may chain up to MPB_MAX_FIELDS fields: header word `next` = words from this header to the next one
    int off = 0;
    for (int f = 0; f < MPB_MAX_FIELDS; ++f) {
        if (!g || n_words - off < MPB_GEOM_HEADER_WORDS) return mpb_failf(MPB_E_INVALID, "%s: geometry buffer too small", __func__);
        const int rc = geom_check_one(g + off, n_words - off, "mpb_geom_check");
        if (rc) return rc;
        const int32_t* gi = reinterpret_cast<const int32_t*>(g + off);
        if (f > 0 && (gi[MPB_GW_KIND] != reinterpret_cast<const int32_t*>(g)[MPB_GW_KIND] || gi[MPB_GW_N_DOF] != reinterpret_cast<const int32_t*>(g)[MPB_GW_N_DOF]))
            return mpb_failf(MPB_E_INVALID, "%s: chained fields must share the robot", __func__);
        const int next = gi[MPB_GW_NEXT];
        if (next == 0) return MPB_OK;
        if (next < gi[MPB_GW_TOTAL] || (next & 3)) return mpb_failf(MPB_E_INVALID, "%s: bad offset to the next field", __func__);
        off += next;
    }
    return mpb_failf(MPB_E_INVALID, "%s: more than MPB_MAX_FIELDS chained fields", __func__);
}

extern "C" int mpb_geom_flags(const float* g, int n_words, int* flags) {
    if (!flags) return mpb_failf(MPB_E_INVALID, "%s: null pointer", __func__);
    *flags = 0;
    const int rc = mpb_geom_check(g, n_words);
    if (rc) return rc;
    int model = -1, max_cells = 0, n_fields = 0;
    bool all_grids = true, all_lists = true;
    for (int off = 0;;) {
        const int32_t* gi = reinterpret_cast<const int32_t*>(g + off);
        const bool is_list = gi[MPB_GW_VERSION] == MPB_GEOM_VERSION_LIST;                                                // (checked above: usable as it stands)
        const bool grid_ok = !is_list && gi[MPB_GW_N_CELLS] > 0 && gi[MPB_GW_N_CELLS] <= MPB_GRID_MAX_CELLS && gi[MPB_GW_N_SPH] <= MPB_GRID_MAX_SPH;   // grid_usable()
        all_grids = all_grids && grid_ok;
        all_lists = all_lists && is_list;
        if (gi[MPB_GW_N_CELLS] > max_cells) max_cells = gi[MPB_GW_N_CELLS];
        ++n_fields;
        const int m = (grid_ok || is_list) ? gi[MPB_GW_MODEL] : 0;
        model = (model < 0 || model == m) ? m : 0;
        if (gi[MPB_GW_NEXT] == 0) break;
        off += gi[MPB_GW_NEXT];
    }
    const int32_t* g0 = reinterpret_cast<const int32_t*>(g);
    const bool point_small = g0[MPB_GW_KIND] == MPB_KIND_POINT && g0[MPB_GW_NEXT] == 0 && g0[MPB_GW_N_SPH] <= 32 && g0[MPB_GW_N_BOX] <= 8;
    *flags = (model > 0 ? (model & MPB_GEOM_FLAG_MODEL_MASK) : 0) | (all_grids ? MPB_GEOM_FLAG_ALL_GRIDS : 0) |
             (point_small ? MPB_GEOM_FLAG_POINT_SMALL : 0) | (g0[MPB_GW_KIND] == MPB_KIND_POINT ? MPB_GEOM_FLAG_POINT : 0) |
             (n_fields == 1 ? MPB_GEOM_FLAG_ONE_FIELD : 0) | (all_lists ? MPB_GEOM_FLAG_ALL_LISTS : 0) |
             ((all_grids || all_lists) ? (max_cells & MPB_GEOM_FLAG_CELLS_MASK) << MPB_GEOM_FLAG_CELLS_SHIFT : 0);
    return MPB_OK;
}

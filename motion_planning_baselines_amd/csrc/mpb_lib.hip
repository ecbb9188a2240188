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

// A buffer tagged with a compile-time robot model (header word 29) must carry exactly that model's tables: the joint
// transforms bit for bit, and as link table the model's collision spheres selected by the keep mask (word 30), of
// which only spheres on frame 1 may be missing.  The model kernels never read these tables -- they trust the tag.
template <class M>
static int model_check_as(const float* g, const char* who) {
    const int32_t* gi = reinterpret_cast<const int32_t*>(g);
    const uint32_t keep = (uint32_t)gi[30];
    if (gi[2] != MPB_KIND_CHAIN || gi[3] != M::N_DOF || gi[4] != M::N_TF) return mpb_failf(MPB_E_INVALID, "%s: model tag does not match the robot", who);
    if (memcmp(g + gi[9], M::TF, sizeof(float) * 12 * M::N_TF) != 0) return mpb_failf(MPB_E_INVALID, "%s: joint transforms differ from the tagged model", who);
    int n = 0;
    for (int l = 0; l < M::N_LINKS; ++l) {
        if (!((keep >> l) & 1u)) {
            if (M::LINK_FRAME[l] != 1) return mpb_failf(MPB_E_INVALID, "%s: only frame-1 spheres of a model may be pruned", who);
            continue;
        }
        if (n >= gi[5]) return mpb_failf(MPB_E_INVALID, "%s: keep mask and link table disagree", who);
        const float* lk = g + gi[10] + 8 * n;
        if (reinterpret_cast<const int32_t*>(lk)[0] != M::LINK_FRAME[l] || memcmp(lk + 1, M::LINK[l], 4 * sizeof(float)) != 0)
            return mpb_failf(MPB_E_INVALID, "%s: link table differs from the tagged model", who);
        ++n;
    }
    if (n != gi[5] || (M::N_LINKS < 32 && (keep >> M::N_LINKS) != 0u)) return mpb_failf(MPB_E_INVALID, "%s: keep mask and link table disagree", who);
    // the model kernels clamp a hinge to [0, 1] (mpb_geom.h, UNIT): margin + largest collision sphere + deepest possible
    // penetration (sphere radius / smallest half extent of a box) must stay below 1
    float rl_max = 0.f, deepest = 0.f;
    for (int l = 0; l < M::N_LINKS; ++l) rl_max = M::LINK[l][3] > rl_max ? M::LINK[l][3] : rl_max;
    for (int o = 0; o < gi[6]; ++o) deepest = g[gi[11] + 4 * o + 3] > deepest ? g[gi[11] + 4 * o + 3] : deepest;
    for (int o = 0; o < gi[7]; ++o) {
        const float* h = g + gi[12] + 8 * o + 4;
        const float m = h[0] < h[1] ? (h[0] < h[2] ? h[0] : h[2]) : (h[1] < h[2] ? h[1] : h[2]);
        deepest = m > deepest ? m : deepest;
    }
    if (!(g[8] + rl_max + deepest < 1.0f)) return mpb_failf(MPB_E_INVALID, "%s: a model-tagged scene must keep every hinge below 1 (margin + radii)", who);
    return MPB_OK;
}

static int model_check(const float* g, const char* who) {
    const int model = reinterpret_cast<const int32_t*>(g)[29];
    if (model == 0) return MPB_OK;
    if (model == PandaModel::ID) return model_check_as<PandaModel>(g, who);
    return mpb_failf(MPB_E_INVALID, "%s: unknown robot model id", who);
}

static int geom_check_one(const float* g, int n_words, const char* who) {
    if (!g || n_words < MPB_GEOM_HEADER_WORDS) return mpb_failf(MPB_E_INVALID, "%s: geometry buffer too small", who);
    const int32_t* gi = reinterpret_cast<const int32_t*>(g);
    if (gi[0] != MPB_GEOM_MAGIC || (gi[1] != MPB_GEOM_VERSION && gi[1] != MPB_GEOM_VERSION_LIST)) return mpb_failf(MPB_E_INVALID, "%s: bad magic/version", who);
    const bool list = gi[1] == MPB_GEOM_VERSION_LIST;       // version 7: the grid section is a list grid (mpb_geom.h, spheres_hinge_list)
    const int kind = gi[2], n_dof = gi[3], n_tf = gi[4], n_links = gi[5], n_sph = gi[6], n_box = gi[7];
    if (kind != MPB_KIND_POINT && kind != MPB_KIND_CHAIN) return mpb_failf(MPB_E_INVALID, "%s: unknown robot kind", who);
    if (n_dof < 1 || n_dof > MPB_MAX_DOF) return mpb_failf(MPB_E_INVALID, "%s: n_dof out of range", who);
    if (kind == MPB_KIND_POINT && (n_dof < 2 || n_dof > 3 || n_links != 1)) return mpb_failf(MPB_E_INVALID, "%s: point robot must be 2-D/3-D with one sphere", who);
    if (kind == MPB_KIND_CHAIN && n_tf != n_dof + 1) return mpb_failf(MPB_E_INVALID, "%s: chain needs n_dof+1 transforms", who);
    if (n_links < 1 || n_sph < 0 || n_box < 0 || n_sph + n_box < 1) return mpb_failf(MPB_E_INVALID, "%s: empty link/obstacle set", who);
    const int off_tf = gi[9], off_links = gi[10], off_sph = gi[11], off_box = gi[12], total = gi[13];
    const int off_cull = gi[14], off_fs = gi[15], off_grid = gi[16];
    const int gnx = gi[17], gny = gi[18], gnz = gi[19], n_cells = gi[26];
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
        // version 6: cells on a lattice through the origin -- lo = (K - 1/2) h per axis with integer K, and header word 31 =
        // Kx + gnx (Ky + gny Kz): what grid_cell_rel (mpb_geom.h) turns round(x / h) into a cell with
        long K[3];
        for (int a = 0; a < 3; ++a) {
            if (!(g[23 + a] > 0.f)) return mpb_failf(MPB_E_INVALID, "%s: bad grid cell size", who);
            const double k = (double)g[20 + a] * (double)g[23 + a] + 0.5;
            K[a] = lrint(k);
            // (lo and 1/h are fp32: their product carries ~|K| 1.2e-7 of rounding, so the tolerance scales with |K| -- an absolute
            // 1e-3 refused the grids build_grid makes beyond |K| ~ 16 700)
            if (fabs(k - (double)K[a]) > 1e-3 + 4e-7 * fabs((double)K[a]) || labs(K[a]) > 100000) return mpb_failf(MPB_E_INVALID, "%s: grid origin is not on the cell lattice", who);
        }
        if ((long)gi[31] != K[0] + (long)gnx * (K[1] + (long)gny * K[2])) return mpb_failf(MPB_E_INVALID, "%s: grid lattice index (word 31) does not match the origin", who);
        if (labs((long)gi[31]) + (long)n_cells >= (1L << 21)) return mpb_failf(MPB_E_INVALID, "%s: grid too far from the origin for the fp32 cell index", who);
    }
    if (list) {   // every cell's candidate range must lie inside the candidate bytes and name existing obstacles
        const unsigned char* cand = reinterpret_cast<const unsigned char*>(g + off_cand);
        const int n_cand = 4 * (total - off_cand);
        for (int i = 0; i < n_cells; ++i) {
            const uint32_t w = (uint32_t)gi[off_grid + i];
            if (w & 0x80000000u) continue;                    // overflowing cell: the kernels test every obstacle
            const int start = (int)(w & 0x7FFFu), ns = (int)((w >> 15) & 0x7Fu), nb = (int)((w >> 22) & 0x3Fu);
            if ((w & 0x70000000u) || ns > MPB_LIST_CELL_MAX_SPH || nb > MPB_LIST_CELL_MAX_BOX || start + ns + nb > n_cand)
                return mpb_failf(MPB_E_INVALID, "%s: list-grid cell out of range", who);
            for (int k = 0; k < ns; ++k)
                if ((int)cand[start + k] >= n_sph) return mpb_failf(MPB_E_INVALID, "%s: grid cell references a missing obstacle", who);
            for (int k = 0; k < nb; ++k)
                if ((int)cand[start + ns + k] >= n_box) return mpb_failf(MPB_E_INVALID, "%s: grid cell references a missing obstacle", who);
        }
    } else
    for (int i = 0; i < n_cells; ++i) {   // every packed obstacle index must exist
        const uint32_t w = (uint32_t)gi[off_grid + i];
        if (w == 0xFFFFFFFEu) continue;
        for (int k = 0; k < 4; ++k) {
            const uint32_t idx = (w >> (8 * k)) & 0xFFu;      // n_sph = unused slot (the far dummy the kernels append)
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
    if (!(g[28] >= 0.f)) return mpb_failf(MPB_E_INVALID, "%s: field scale must be >= 0", who);
    return model_check(g, who);
}


extern "C" int mpb_geom_check(const float* g, int n_words) {
    // a buffer may chain up to MPB_MAX_FIELDS fields: header word 27 = words from this header to the next one
    int off = 0;
    for (int f = 0; f < MPB_MAX_FIELDS; ++f) {
        if (!g || n_words - off < MPB_GEOM_HEADER_WORDS) return mpb_failf(MPB_E_INVALID, "%s: geometry buffer too small", __func__);
        const int rc = geom_check_one(g + off, n_words - off, "mpb_geom_check");
        if (rc) return rc;
        const int32_t* gi = reinterpret_cast<const int32_t*>(g + off);
        if (f > 0 && (gi[2] != reinterpret_cast<const int32_t*>(g)[2] || gi[3] != reinterpret_cast<const int32_t*>(g)[3]))
            return mpb_failf(MPB_E_INVALID, "%s: chained fields must share the robot", __func__);
        const int next = gi[27];
        if (next == 0) return MPB_OK;
        if (next < gi[13] || (next & 3)) return mpb_failf(MPB_E_INVALID, "%s: bad offset to the next field", __func__);
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
        const bool is_list = gi[1] == MPB_GEOM_VERSION_LIST;                                                // (checked above: usable as it stands)
        const bool grid_ok = !is_list && gi[26] > 0 && gi[26] <= MPB_GRID_MAX_CELLS && gi[6] <= MPB_GRID_MAX_SPH;   // grid_usable()
        all_grids = all_grids && grid_ok;
        all_lists = all_lists && is_list;
        if (gi[26] > max_cells) max_cells = gi[26];
        ++n_fields;
        const int m = (grid_ok || is_list) ? gi[29] : 0;
        model = (model < 0 || model == m) ? m : 0;
        if (gi[27] == 0) break;
        off += gi[27];
    }
    const int32_t* g0 = reinterpret_cast<const int32_t*>(g);
    const bool point_small = g0[2] == MPB_KIND_POINT && g0[27] == 0 && g0[6] <= 32 && g0[7] <= 8;
    *flags = (model > 0 ? (model & 0xFF) : 0) | (all_grids ? 0x100 : 0) | (point_small ? 0x200 : 0) |
             (g0[2] == MPB_KIND_POINT ? 0x400 : 0) | (n_fields == 1 ? 0x1000 : 0) | (all_lists ? 0x2000 : 0) |
             ((all_grids || all_lists) ? (max_cells & 0x1FFF) << 16 : 0);
    return MPB_OK;
}

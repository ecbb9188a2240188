// mpb_sdf_host.h -- host side shared by the translation units that launch on a packed SDF-grid buffer (mpb_sdf_grid.hip: sample, cost,
// gradient, predicate and the builders from primitives and occupancy; mpb_sdf_mesh.hip: the builder from triangle meshes): the header
// check and the cached header read.  No device code.
#pragma once
#include <math.h>

#include "mpb_host.h"
#include "../../include/mpb_sdf_layout.h"
#include "../../include/mpb_mesh_layout.h"

// header, offsets and limits (n_words < 0: the total is not compared with a word count)
static int sdf_header_check(const int32_t* si, long long n_words, const char* who) {
    if (si[MPB_DW_MAGIC] != MPB_SDF_MAGIC || si[MPB_DW_VERSION] != MPB_SDF_VERSION) return mpb_failf(MPB_E_INVALID, "%s: bad magic/version of the SDF-grid buffer", who);
    const int kind = si[MPB_DW_KIND], n_dof = si[MPB_DW_N_DOF], n_tf = si[MPB_DW_N_TF], n_links = si[MPB_DW_N_LINKS];
    const int nx = si[MPB_DW_DIMS], ny = si[MPB_DW_DIMS + 1], nz = si[MPB_DW_DIMS + 2];
    if (kind != MPB_KIND_POINT && kind != MPB_KIND_CHAIN) return mpb_failf(MPB_E_INVALID, "%s: unknown robot kind %d", who, kind);
    if (n_dof < 1 || n_dof > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "%s: n_dof = %d outside 1..MPB_MAX_DOF = %d", who, n_dof, MPB_MAX_DOF);
    if (n_links < 1 || n_links > MPB_SDF_MAX_LINKS) return mpb_failf(MPB_E_UNSUPPORTED, "%s: %d collision spheres outside 1..MPB_SDF_MAX_LINKS = %d", who, n_links, MPB_SDF_MAX_LINKS);
    if (nx < 2 || ny < 2 || nz < 1 || nx > MPB_SDF_MAX_DIM || ny > MPB_SDF_MAX_DIM || nz > MPB_SDF_MAX_DIM)
        return mpb_failf(MPB_E_UNSUPPORTED, "%s: grid of %d x %d x %d nodes: a dimension outside 2..MPB_SDF_MAX_DIM = %d (nz: 1 = planar)", who, nx, ny, nz, MPB_SDF_MAX_DIM);
    const long long n_nodes = (long long)nx * ny * nz;
    if (n_nodes > MPB_SDF_MAX_NODES) return mpb_failf(MPB_E_UNSUPPORTED, "%s: %lld nodes exceed MPB_SDF_MAX_NODES = %d", who, n_nodes, MPB_SDF_MAX_NODES);
    if (kind == MPB_KIND_CHAIN ? (n_tf != n_dof + 1) : (n_tf != 0 || n_links != 1 || n_dof > 3 || n_dof < 2))
        return mpb_failf(MPB_E_INVALID, "%s: a chain needs n_dof + 1 transforms, a point robot none, one sphere and 2 or 3 coordinates", who);
    if (kind == MPB_KIND_CHAIN && nz == 1) return mpb_failf(MPB_E_INVALID, "%s: a planar grid (nz = 1) serves point robots only", who);
    const int off_tf = si[MPB_DW_OFF_TF], off_links = si[MPB_DW_OFF_LINKS], off_nodes = si[MPB_DW_OFF_NODES], total = si[MPB_DW_TOTAL];
    const int want_nodes = (off_links + 8 * n_links + MPB_SDF_NODE_ALIGN - 1) / MPB_SDF_NODE_ALIGN * MPB_SDF_NODE_ALIGN;
    if (off_tf != MPB_SDF_HEADER_WORDS || off_links != off_tf + 12 * n_tf || off_nodes != want_nodes || (long long)total != off_nodes + n_nodes ||
        (n_words >= 0 && total != n_words))
        return mpb_failf(MPB_E_INVALID, "%s: inconsistent section offsets / total of the SDF-grid buffer", who);
    const float* sf = reinterpret_cast<const float*>(si);
    const float cell = sf[MPB_DW_CELL], inv = sf[MPB_DW_INV_CELL], margin = sf[MPB_DW_MARGIN];
    if (!(cell > 0.f && cell < 3.0e38f) || inv != 1.0f / cell) return mpb_failf(MPB_E_INVALID, "%s: cell must be positive and finite, inv_cell its fp32 reciprocal", who);
    if (!(fabsf(margin) < 3.0e38f) || !(fabsf(sf[MPB_DW_LO]) < 3.0e38f) || !(fabsf(sf[MPB_DW_LO + 1]) < 3.0e38f) || !(fabsf(sf[MPB_DW_LO + 2]) < 3.0e38f))
        return mpb_failf(MPB_E_INVALID, "%s: margin and lo must be finite", who);
    return MPB_OK;
}

// what a launch needs of a device buffer's header (every node index comes from the dims), through the cache of mpb_host.h (its contract
// is stated there); mpb_sdf_grid_invalidate drops the entry of an address that gets another buffer
struct SdfShape { const void* ptr; int dev, kind, n_dof, n_links, nx, ny, nz; float lo[3], cell; };
inline MpbHeaderCache<SdfShape, MPB_SDF_HEADER_WORDS> g_sdf_cache;   // (inline: ONE table for the translation units that include this)

static int sdf_shape(const float* sdfb, SdfShape& out, const char* who) {
    return g_sdf_cache.get(sdfb, out, who, "SDF-grid", [who](const int32_t* hdr, SdfShape& S) {
        S.kind = hdr[MPB_DW_KIND], S.n_dof = hdr[MPB_DW_N_DOF], S.n_links = hdr[MPB_DW_N_LINKS];
        S.nx = hdr[MPB_DW_DIMS], S.ny = hdr[MPB_DW_DIMS + 1], S.nz = hdr[MPB_DW_DIMS + 2];
        const float* hf = reinterpret_cast<const float*>(hdr);
        S.lo[0] = hf[MPB_DW_LO], S.lo[1] = hf[MPB_DW_LO + 1], S.lo[2] = hf[MPB_DW_LO + 2], S.cell = hf[MPB_DW_CELL];
        return sdf_header_check(hdr, -1, who);
    });
}

// the same for a packed mesh buffer (mpb_sdf_mesh.hip parses it); here because mpb_sdf_grid_invalidate drops an address from both tables
struct MeshShape { const void* ptr; int dev, n_tri, n_groups, is_signed, off_tris, off_boxes; float thickness, max_abs; };
inline MpbHeaderCache<MeshShape, MPB_MESH_HEADER_WORDS> g_mesh_cache;

// mpb_self_host.h -- host side shared by the translation units that launch on a packed self-collision buffer (mpb_self_collision.hip:
// cost, gradient, predicate; the world launchers of mpb_world_host.h): the header check and the cached header read.  No device code.
#pragma once
#include "mpb_host.h"
#include "../../include/mpb_self_layout.h"

// header, offsets and limits (n_words < 0: the total is not compared with a word count)
static int self_header_check(const int32_t* si, int n_words, const char* who) {
    if (si[MPB_SW_MAGIC] != MPB_SELF_MAGIC || si[MPB_SW_VERSION] != MPB_SELF_VERSION) return mpb_failf(MPB_E_INVALID, "%s: bad magic/version of the self-collision buffer", who);
    const int n_dof = si[MPB_SW_N_DOF], n_tf = si[MPB_SW_N_TF], n_links = si[MPB_SW_N_LINKS], n_pairs = si[MPB_SW_N_PAIRS];
    if (n_dof < 1 || n_dof > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "%s: n_dof = %d outside 1..MPB_MAX_DOF = %d", who, n_dof, MPB_MAX_DOF);
    if (n_links < 2 || n_links > MPB_SELF_MAX_LINKS) return mpb_failf(MPB_E_UNSUPPORTED, "%s: %d collision spheres outside 2..MPB_SELF_MAX_LINKS = %d", who, n_links, MPB_SELF_MAX_LINKS);
    if (n_pairs < 0 || n_pairs > MPB_SELF_MAX_PAIRS) return mpb_failf(MPB_E_UNSUPPORTED, "%s: %d pairs outside 0..MPB_SELF_MAX_PAIRS = %d", who, n_pairs, MPB_SELF_MAX_PAIRS);
    if (n_tf != n_dof + 1) return mpb_failf(MPB_E_INVALID, "%s: a chain needs n_dof + 1 transforms", who);
    const int off_tf = si[MPB_SW_OFF_TF], off_links = si[MPB_SW_OFF_LINKS], off_pairs = si[MPB_SW_OFF_PAIRS], total = si[MPB_SW_TOTAL];
    if (off_tf != MPB_SELF_HEADER_WORDS || off_links != off_tf + 12 * n_tf || off_pairs != off_links + 8 * n_links ||
        total != off_pairs + MPB_SELF_PAIR_WORDS * n_pairs || (n_words >= 0 && total != n_words))
        return mpb_failf(MPB_E_INVALID, "%s: inconsistent section offsets / total of the self-collision buffer", who);
    return MPB_OK;
}

// what a launch needs of a device buffer's header (LDS bytes come from n_links), through the cache of mpb_host.h (its contract is stated
// there); memory that gets ANOTHER buffer at an address an earlier call has seen must be announced with mpb_self_invalidate
struct SelfShape { const void* ptr; int dev, n_dof, n_links, n_pairs; };
inline MpbHeaderCache<SelfShape, MPB_SELF_HEADER_WORDS> g_self_cache;   // (inline: ONE table for the translation units that include this)

static int self_shape(const float* selfb, SelfShape& out, const char* who) {
    return g_self_cache.get(selfb, out, who, "self-collision", [who](const int32_t* hdr, SelfShape& S) {
        S.n_dof = hdr[MPB_SW_N_DOF], S.n_links = hdr[MPB_SW_N_LINKS], S.n_pairs = hdr[MPB_SW_N_PAIRS];
        return self_header_check(hdr, -1, who);
    });
}

// LDS of a launch ([L][3][64] words, twice with gradients), the kernel's limit raised where that takes it
static int self_lds_bytes(const void* kernel, const SelfShape& S, bool grad, size_t& bytes, const char* who) {
    bytes = (size_t)S.n_links * 192 * sizeof(float) * (grad ? 2 : 1);
    return mpb_raise_lds_limit(kernel, S.dev, bytes, who);
}

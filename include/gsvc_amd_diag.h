/*
 * gsvc_amd_diag.h -- entry points of the DIAGNOSTIC library only
 * (gsvc_amd/lib/libgsvc_amd_diag.so, built from the same sources with
 * -DGSVC_DIAG).  The product library libgsvc_amd.so has none of these: its
 * kernel selection depends only on the call's arguments and the data, and it
 * carries no diagnostic kernel variants.  tools/ (microbenchmarks, A/B runs,
 * timestamped variants) and the variant-comparison tests load the diagnostic
 * library (gsvc_amd._lib.diagnostic()); nothing in the product path does.
 * Not part of the reference interface.
 */
#ifndef GSVC_AMD_DIAG_H
#define GSVC_AMD_DIAG_H

#include "gsvc_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The knobs of gsvc_debug_set: every one is 0 in production.  "exact": the
 * results stay equal; "ablation": a phase is skipped, the results are wrong
 * (timing experiments only).  gsvc_amd/knobs.py mirrors this enum
 * (tests/test_capi.py holds the two together); DESIGN.md §1c has the table of
 * who uses which. */
enum gsvc_knob {
    GSVC_KNOB_FWD_MODE = 0,          /* sum-forward kernel mode: 1 sparse, 2 banded, 6 per-tile choice, 9 id slabs (exact); 3, 7 timestamped; 4, 5 ablations */
    GSVC_KNOB_SPARSE_MAX = 3,        /* v > 0: entries per tile up to which modes 3 / 6 take the sparse path (default 8); exact */
    GSVC_KNOB_STAMP = 5,             /* timestamps into the gsvc_debug_set_ptr buffer: 1 projection waves, 2 wg256 tile kernel, 3 band tile kernel, 4 splat kernel waves; exact */
    GSVC_KNOB_TILE_WG256 = 8,        /* 1: the training step's 256-thread workgroup-per-tile kernel instead of the band kernel; exact */
    GSVC_KNOB_TILE_ABLATE = 13,      /* band tile kernel bits: 2 no backward, 4 no forward blend, 8 no backward pixel work, 16 no run sums, 32 no atomics, 256 no v_out reads (ablations); 64 entry order, 128 readlane ranking (exact) */
    GSVC_KNOB_TILE_NO_GROUPS = 14,   /* 1: band tile kernel forward without the lane-group lists; exact */
    GSVC_KNOB_GROUP_MIN = 15,        /* v > 0: sum-forward chunks of <= v - 1 entries skip the lane-group lists (default 24); exact */
    GSVC_KNOB_NO_SIGMA_CUT = 19,     /* 1: sparse render chunks never take the sigma-threshold blend; exact */
    GSVC_KNOB_RECORD_SLABS = 24,     /* 1: the single-frame render over 48-byte record slabs, not id slabs; exact */
    GSVC_KNOB_BATCH_ID_SLABS = 25,   /* 1: batched frames render over id slabs too; exact */
    GSVC_KNOB_KEEP_ORDER = 27,       /* 1: the ordered projection at any density (no plain projection of sparse frames); exact */
    GSVC_KNOB_ALPHA_BWD_ABLATE = 30, /* alpha backward: 1, 2 skip phases of the kernel; ablation */
    GSVC_KNOB_SPARSE_ABLATE = 36,    /* sparse composite bits: 1 no blend, 2 no stores, 4 no record loads, 8 no ranking, 16 no loads at all; ablation */
    GSVC_KNOB_GENERIC_RENDER = 38,   /* 1: the single-frame render by the generic id-slab kernel, not the two-tile one; exact */
    GSVC_KNOB_RENDER_STAMPS = 39     /* 1: the id-slab composite stamps its phases into the gsvc_debug_set_ptr buffer; exact */
};
/* Retired, never reuse (their A/Bs are finished; DESIGN.md §1c names the
 * section that holds each verdict): 1, 2, 4, 6, 7, 9, 10, 11, 12, 16, 17, 18,
 * 20, 21, 22, 23, 26, 28, 29, 31, 32, 33, 34, 35, 37. */

/* Sets knob ``key`` (an enum gsvc_knob) and returns its previous value; -1
 * for any key that is not a live enumerator, retired numbers included. */
int gsvc_debug_set(int key, int value);
/* Device buffer the timestamped variants write into (int64 per tile x 4). */
void gsvc_debug_set_ptr(void *ptr);

#ifdef __cplusplus
}
#endif

#endif /* GSVC_AMD_DIAG_H */

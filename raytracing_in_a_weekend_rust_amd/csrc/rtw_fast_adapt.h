// rtw_fast_adapt.h -- adaptive fast mode (rtw_fast_adapt.hip): samples added to the pixels
// of a device list, per-pixel counts and luminance moments beside the sums, the selection
// of the pixels that still need samples, and the resolve by per-pixel counts. The
// definitions (moments, sample order, convergence test, selection) are in rtw_capi.h.
#pragma once

#include "rtw_fast.h"

namespace rtw_fast {

// Ordinals [counts[p], min(counts[p] + m, f.n_off)) of every listed pixel p: ordinal i is
// lattice sample (i * k_mul) mod f.n_off. f.out is unused; f.n_off <= 65535.
struct ListParams {
    FastParams f;
    const uint32_t *list;    // shard-local pixel indices, each at most once; null: every pixel
    const uint32_t *n_list;  // the list's length, on the device (not read with a null list)
    uint32_t m, k_mul;       // k_mul < max(f.n_off, 2), coprime to f.n_off
    uint32_t chunk;          // most list entries a wave claims per cursor atomic (set by the launcher)
    unsigned long long *acc;  // n_rows x W x 3 u64
    unsigned long long *mom;  // n_rows x W x 2 u64: sum q, sum q^2
    uint32_t *counts;         // n_rows x W u32
};

constexpr uint32_t kListRing = 8;  // pixels a wave keeps in flight
constexpr uint32_t kListSums = 5;  // R, G, B, q, q^2
// two workgroups per CU with the ring sums (8 waves x kListRing x kListSums u64) beside them
constexpr uint32_t kListLdsCap = 80 * 1024 - (kBlock / 64) * kListRing * kListSums * 8;

// Enqueues the accumulation. Zeroes the cursor and f.counters[0..5] first; [2] ends as
// n_rows * W when every list entry was served (the latch's test), [5] as the samples traced.
hipError_t launch_accumulate_list(const ListParams &A, int n_cu, hipStream_t st, bool scene_lds = true);

// Sums to the f32 mean frame and/or the RGBA8 preview with the divisor counts[p] (0: the
// pixel resolves to 0). full (nullable): += the number of pixels with counts[p] >= n_off.
hipError_t launch_resolve_counts(const unsigned long long *acc, const uint32_t *counts, uint64_t n_pixels,
                                 float *out_rgb, uint32_t *preview_rgba8, uint32_t n_off, unsigned long long *full,
                                 hipStream_t st);

}  // namespace rtw_fast

namespace rtw {
void adapt_shutdown();  // frees the selection's per-device scratch (rtw_shutdown)
}

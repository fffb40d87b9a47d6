// rtw_fast_denoise.h -- the guided a-trous filter of fast-mode frames (rtw_fast_denoise.hip):
// first-hit guides (normal + sphere tag) traced by a persistent kernel, and the filter that
// spends them and the adaptive buffers' luminance moments. The definitions (guide record,
// prepare, level, weights) are in rtw_capi.h; the design is DESIGN 3.12.
#pragma once

#include "rtw_capi.h"
#include "rtw_fast.h"

namespace rtw_fast {

// One 16-byte record per shard pixel from the centre ray. f is fast_params at samples_sqrt = 0
// with f.defocus = 0 (start_path's pixel-centre ray from look_from, no draw); f.out is unused.
struct GuideParams {
    FastParams f;
    float4 *guides;             // n_rows x W records
    uint32_t tiles_x, n_tiles;  // 8x8 pixel tiles per row of tiles, and in all
};

// Enqueues the guides (zeroes the cursor and f.counters[0..4] first; [0] and [2] end as the
// number of pixels).
hipError_t launch_guides(const GuideParams &A, int n_cu, hipStream_t st, bool scene_lds = true);

}  // namespace rtw_fast

namespace rtw {
// rtw_denoise_fast's checks of its parameter block (NULL: the defaults); returns the block to use.
rtw_denoise_params checked_denoise_params(const rtw_denoise_params *p);
void denoise_shutdown();  // frees the filter's per-device planes (rtw_shutdown)
}  // namespace rtw

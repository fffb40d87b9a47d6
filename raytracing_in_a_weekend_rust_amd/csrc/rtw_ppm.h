// rtw_ppm.h -- the device output stage (rtw_ppm.hip): a framebuffer in HBM to RGB8
// and to the reference's P3 text (Color::wire_full_file, color.rs:196-247), with the
// host writer's bytes for every input. Geometry shared by the kernels and their
// launch code; see DESIGN.md 3.8.
#pragma once

#include <cstdint>

namespace rtw {

constexpr uint32_t kPpmBlock = 256;                          // threads per workgroup (4 waves)
constexpr uint32_t kPpmPack = 4;                             // channels per lane and step: one u32 of RGB8
constexpr uint32_t kPpmSubs = 4;                             // steps per tile
constexpr uint32_t kPpmTile = kPpmBlock * kPpmPack * kPpmSubs;  // 4096 channels per tile
constexpr uint32_t kPpmMaxLen = 4;                           // "255" + separator
constexpr uint32_t kPpmStage = kPpmTile * kPpmMaxLen + 16;   // LDS text stage: a tile + the 16 B phase
constexpr uint32_t kPpmScanBlock = 1024;                     // the one workgroup of rtw_ppm_scan
constexpr uint64_t kPpmMaxChannels = 1ull << 40;             // limit of this build

// Frees the per-device contexts (table, RGB8, counts, offsets, text). rtw_shutdown calls it.
void ppm_shutdown();

}  // namespace rtw

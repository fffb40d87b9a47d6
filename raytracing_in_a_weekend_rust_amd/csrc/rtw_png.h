// rtw_png.h -- the device PNG encoder (rtw_png.hip): an RGB8 image in HBM to a
// complete PNG file (8-bit, colour type 2, one IDAT) in a device buffer. Geometry
// shared by the kernels and their launch code; see DESIGN.md 3.9.
#pragma once

#include <cstdint>

namespace rtw {

constexpr uint32_t kPngBlock = 256;  // threads per workgroup (4 waves)
constexpr uint32_t kPngItems = 8;    // filtered bytes per lane
// Filtered bytes per tile, i.e. per deflate block. At most kPngTile literals + the
// end-of-block symbol = 2049 symbols: below the 2584 (Fibonacci) a Huffman code needs
// to reach 16 bits, so the code lengths never have to be limited.
constexpr uint32_t kPngTile = kPngBlock * kPngItems;
static_assert(kPngTile + 1 < 2584, "a tile's Huffman code must fit 15 bits without length limiting");
constexpr uint32_t kPngStoredHead = 5;                         // BFINAL/BTYPE byte + LEN + NLEN
constexpr uint32_t kPngTileMax = kPngTile + kPngStoredHead;    // no tile's block(s) are larger
constexpr uint32_t kPngStage = (kPngTileMax + 16 + 15) / 16 * 16 + 16;  // LDS stage: a tile + the 16 B phase + slack
constexpr uint32_t kPngCrcChunk = 9;                           // bytes per lane of the tile CRC: 256 * 9 >= kPngTileMax
static_assert(kPngBlock * kPngCrcChunk >= kPngTileMax, "the tile CRC covers the largest tile");
constexpr uint32_t kPngLitLen = 286, kPngLens = 288;           // lit/len code lengths + the two distance codes
constexpr uint32_t kPngHead = 8 + 25 + 8 + 2;                  // signature, IHDR chunk, IDAT length + type, zlib header
constexpr uint32_t kPngTail = 4 + 4 + 12;                      // Adler-32, IDAT CRC, IEND chunk
constexpr uint32_t kPngScanBlock = 1024;                       // the one workgroup of the scan and of the finish
constexpr uint64_t kPngMaxStream = 0x7fffffffull;              // one IDAT: its length field is 31 bits

// Frees the per-device contexts. rtw_shutdown reaches it through ppm_shutdown.
void png_shutdown();

}  // namespace rtw

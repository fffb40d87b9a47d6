// rtw_png.hip -- the device PNG encoder: an RGB8 image in HBM (a caller's, or the one
// rtw_quantise_device makes of a rendered frame) becomes a complete PNG file in a device
// buffer: signature, IHDR (8-bit, colour type 2), one IDAT holding one zlib stream, IEND.
// Integer and byte work only. DESIGN.md 3.9.
//
// Deflate is a serial bit stream; it is made parallel by cutting the filtered stream
// (H rows of 1 + 3W bytes: the filter type, then the residuals) into tiles of kPngTile
// bytes. A workgroup encodes a tile as a deflate block of its own whose matches never
// leave the tile, and every tile but the last ends with an empty stored block, which
// pads it to a byte boundary: a tile's bytes depend on that tile alone, and the tiles
// concatenate at byte offsets that one scan hands out.
//
// Tokens are zlib's Z_RLE: literals and distance-1 matches. A run of k equal bytes is
// a literal, matches of 258, a match of the rest (>= 3) or 1-2 more literals; the runs
// come from two block-wide scans (last run start at or before, first run start after),
// so the token that starts at a byte is a function of that byte's run alone.
//
// Codes: one dynamic-Huffman block per tile. The literal/length histogram is built with
// LDS atomics, rank-sorted, merged by the two-queue method and read back as depths. A
// tile holds at most kPngTile + 1 = 2049 symbols, fewer than the 2584 a 16-bit code
// needs, so the lengths are never limited (rtw_png.h). The one distance symbol is sent
// as a complete two-code tree, the code-length code is a fixed complete code, and zero
// runs of the length table use its symbols 17 and 18. A tile whose exact size is not
// below the stored form's is stored.
//
// Launches, all on the caller's stream, none waiting on another workgroup:
//   rtw_png_filter   one wave per row: filter 0/1/2 with the least sum of |residual|
//   rtw_png_plan     per tile: filter into LDS, runs, histogram, code lengths, exact
//                    size, Adler-32 partial -> the tile's record and length table
//   rtw_png_scan     one workgroup: tile offsets, the Adler-32, counters
//   rtw_png_emit     per tile: token bit offsets by a scan, codes OR-ed into an LDS bit
//                    buffer at the destination's 16-byte phase, aligned 16-byte stores,
//                    and the CRC-32 of the tile's bytes
//   rtw_png_finish   one workgroup: the IDAT CRC = xor of every tile's CRC times
//                    x^(8 * bytes after it) in GF(2)[x] mod the CRC polynomial; header,
//                    Adler-32, CRC and IEND
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <map>
#include <mutex>
#include <string>

#include "rtw_capi.h"
#include "rtw_host.h"
#include "rtw_internal.h"
#include "rtw_png.h"

namespace {

using rtw::kPngBlock;
using rtw::kPngHead;
using rtw::kPngItems;
using rtw::kPngLens;
using rtw::kPngLitLen;
using rtw::kPngStage;
using rtw::kPngTile;
constexpr uint32_t kWave = 64;
constexpr uint32_t kCrcPoly = 0xedb88320u;  // reflected: bit 31 is x^0
constexpr uint32_t kAdlerMod = 65521;
constexpr uint32_t kPrefixBits = 3 + 5 + 5 + 4 + 19 * 3;  // block header up to the length table
constexpr uint32_t kStoredFlag = 1u << 31;
// control words of a call
constexpr uint32_t kCtlEnd = 0, kCtlAdler = 1, kCtlStored = 2, kCtlRows = 3, kCtlCrc = 6, kCtlWords = 8;
// a token in a register: symbol, extra-bit count, extra bits, "is a match", "starts here"
constexpr uint32_t kTokEbShift = 9, kTokExtraShift = 12, kTokMatch = 1u << 20, kTokValid = 1u << 31;

// Built once on the host (png_tables) and staged in LDS by the kernels that need them.
struct PngTables {
    uint32_t crc[256];     // the byte-wise CRC-32 table
    uint32_t pw[256];      // x^(8 * kPngCrcChunk * t)
    uint32_t x2n[32];      // x^(2^n)
    uint32_t cl_code[19];  // the fixed code-length code, bit-reversed
    uint32_t cl_len[19];
    uint32_t prefix[3];    // BTYPE = 2, HLIT = 29, HDIST = 1, HCLEN = 15 and the 19 lengths (BFINAL clear)
};

struct PngHeader {
    uint8_t s[48];      // signature, IHDR chunk, IDAT length (filled on the device) + type, zlib header
    uint32_t crc_head;  // CRC-32 of "IDAT" + the zlib header
};

// a * b in GF(2)[x] modulo the CRC polynomial
__host__ __device__ inline uint32_t multmodp(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) {
            p ^= b;
            if (!(a & (m - 1))) break;
        }
        b = b & 1 ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
// x^(8 * k)
__host__ __device__ inline uint32_t xpow8(const uint32_t *x2n, uint64_t k) {
    uint32_t p = 1u << 31;
    for (uint32_t i = 3; k; k >>= 1, ++i)
        if (k & 1) p = multmodp(x2n[i & 31], p);
    return p;
}
__host__ __device__ inline uint32_t crc_bytes(const uint32_t *tab, const uint8_t *p, uint32_t n) {
    uint32_t c = ~0u;
    for (uint32_t i = 0; i < n; ++i) c = tab[(c ^ p[i]) & 255u] ^ (c >> 8);
    return ~c;
}

// ---- workgroup-wide primitives (every thread of the block calls; ws: one word per wave) ----
__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
    for (uint32_t m = kWave / 2; m; m >>= 1) x += __shfl_xor(x, m, kWave);
    return x;
}
__device__ __forceinline__ uint32_t wave_xor(uint32_t x) {
#pragma unroll
    for (uint32_t m = kWave / 2; m; m >>= 1) x ^= __shfl_xor(x, m, kWave);
    return x;
}
enum Op { kSum, kXor };
template <Op OP>
__device__ __forceinline__ uint32_t block_reduce(uint32_t x, uint32_t *ws) {
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, nw = blockDim.x / kWave;
    x = OP == kSum ? wave_sum(x) : wave_xor(x);
    __syncthreads();  // ws may still be read from the previous use
    if (lane == 0) ws[wave] = x;
    __syncthreads();
    uint32_t r = 0;
    for (uint32_t w = 0; w < nw; ++w) r = OP == kSum ? r + ws[w] : r ^ ws[w];
    return r;
}
// exclusive prefix sum over the block's threads; all = the block's total
__device__ __forceinline__ uint32_t block_excl_sum(uint32_t x, uint32_t *ws, uint32_t &all) {
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, nw = blockDim.x / kWave;
    uint32_t inc = x;
#pragma unroll
    for (uint32_t d = 1; d < kWave; d <<= 1) {
        const uint32_t y = __shfl_up(inc, d, kWave);
        if (lane >= d) inc += y;
    }
    __syncthreads();
    if (lane == kWave - 1) ws[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    all = 0;
    for (uint32_t w = 0; w < nw; ++w) {
        const uint32_t a = ws[w];
        before += w < wave ? a : 0u;
        all += a;
    }
    return before + inc - x;
}
// max of x over the threads before this one (0 if none)
__device__ __forceinline__ uint32_t block_excl_max(uint32_t x, uint32_t *ws) {
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    uint32_t inc = x;
#pragma unroll
    for (uint32_t d = 1; d < kWave; d <<= 1) {
        const uint32_t y = __shfl_up(inc, d, kWave);
        if (lane >= d) inc = max(inc, y);
    }
    uint32_t r = __shfl_up(inc, 1, kWave);
    if (lane == 0) r = 0;
    __syncthreads();
    if (lane == kWave - 1) ws[wave] = inc;
    __syncthreads();
    for (uint32_t w = 0; w < wave; ++w) r = max(r, ws[w]);
    return r;
}
// min of x over the threads after this one (~0 if none)
__device__ __forceinline__ uint32_t block_excl_min_after(uint32_t x, uint32_t *ws) {
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, nw = blockDim.x / kWave;
    uint32_t inc = x;
#pragma unroll
    for (uint32_t d = 1; d < kWave; d <<= 1) {
        const uint32_t y = __shfl_down(inc, d, kWave);
        if (lane + d < kWave) inc = min(inc, y);
    }
    uint32_t r = __shfl_down(inc, 1, kWave);
    if (lane == kWave - 1) r = ~0u;
    __syncthreads();
    if (lane == 0) ws[wave] = inc;
    __syncthreads();
    for (uint32_t w = wave + 1; w < nw; ++w) r = min(r, ws[w]);
    return r;
}

// The segmented scan: for the ITEMS consecutive elements a thread owns of v[0, n), the
// first index of the run of equal values each lies in, and the index one past its end.
template <uint32_t ITEMS>
__device__ __forceinline__ void run_bounds(const uint8_t *v, uint32_t n, uint32_t *ws, uint32_t start[ITEMS],
                                           uint32_t end[ITEMS]) {
    const uint32_t base = threadIdx.x * ITEMS;
    bool head[ITEMS];  // a run starts here; so it does at every index past the data
    uint32_t last = 0, first = ~0u;
#pragma unroll
    for (uint32_t j = 0; j < ITEMS; ++j) {
        const uint32_t i = base + j;
        head[j] = i >= n || i == 0 || v[i] != v[i - 1];
        if (head[j]) last = i, first = min(first, i);
    }
    uint32_t cur = block_excl_max(last, ws);
    uint32_t nxt = block_excl_min_after(first, ws);
#pragma unroll
    for (uint32_t j = 0; j < ITEMS; ++j) {
        if (head[j]) cur = base + j;
        start[j] = cur;
    }
#pragma unroll
    for (uint32_t j = ITEMS; j-- > 0;) {
        end[j] = min(nxt, n);
        if (head[j]) nxt = base + j;
    }
}

// The length symbol of a match of len bytes (3..258), its extra-bit count and bits.
__device__ __forceinline__ uint32_t match_token(uint32_t len) {
    if (len == 258) return 285u | kTokMatch | kTokValid;
    const uint32_t l = len - 3;
    if (l < 8) return (257u + l) | kTokMatch | kTokValid;
    const uint32_t eb = 29u - __clz(l);  // floor(log2 l) - 2
    const uint32_t sym = 261u + 4u * eb + ((l >> eb) & 3u);
    return sym | (eb << kTokEbShift) | ((l & ((1u << eb) - 1u)) << kTokExtraShift) | kTokMatch | kTokValid;
}
// The token that starts at offset p of a run of k bytes of value b (0: none starts there).
__device__ __forceinline__ uint32_t tile_token(uint32_t b, uint32_t p, uint32_t k) {
    const uint32_t lit = b | kTokValid;
    if (p == 0) return lit;
    const uint32_t r = k - 1, q = p - 1, full = r / 258u, tail = full * 258u, rem = r - tail;
    if (q < tail) return q % 258u == 0 ? match_token(258) : 0u;
    if (rem >= 3) return q == tail ? match_token(rem) : 0u;
    return lit;
}
__device__ __forceinline__ uint32_t tok_sym(uint32_t t) { return t & 511u; }
__device__ __forceinline__ uint32_t tok_eb(uint32_t t) { return (t >> kTokEbShift) & 7u; }
// bits of a token beyond its symbol's code: the length's extra bits and the 1-bit distance code
__device__ __forceinline__ uint32_t tok_more(uint32_t t) { return t & kTokMatch ? tok_eb(t) + 1u : 0u; }

// The token of the length table that starts at offset p of a run of k entries of value v:
// symbol | extra-bit count << 8 | extra bits << 16 | kTokValid (0: none starts there).
// Zero runs become 18s (11..138 zeros) and 17s (3..10); other lengths are sent as they are.
__device__ __forceinline__ uint32_t table_token(uint32_t v, uint32_t p, uint32_t k) {
    if (v) return v | kTokValid;
    const uint32_t full = k / 138u, tail = full * 138u, rem = k - tail;
    if (p < tail) return p % 138u == 0 ? (18u | 7u << 8 | 127u << 16 | kTokValid) : 0u;
    if (rem >= 11) return p == tail ? (18u | 7u << 8 | (rem - 11u) << 16 | kTokValid) : 0u;
    if (rem >= 3) return p == tail ? (17u | 3u << 8 | (rem - 3u) << 16 | kTokValid) : 0u;
    return kTokValid;
}

// Filtered bytes [tile * kPngTile, +n) into fb. Every byte needs only raw RGB8 values
// (itself, the pixel to its left, the row above), so a tile never waits for another.
__device__ __forceinline__ void load_filtered(const uint8_t *__restrict__ img, const uint8_t *__restrict__ ftype,
                                              uint32_t w3, uint32_t tile, uint32_t n, uint8_t *fb) {
    const uint32_t local = threadIdx.x * kPngItems;
    if (local >= n) return;
    const uint32_t rowlen = w3 + 1, g0 = tile * kPngTile + local;
    uint32_t row = g0 / rowlen, c = g0 - row * rowlen;
    uint32_t f = ftype[row];
    const uint8_t *p = img + static_cast<size_t>(row) * w3;
    const uint32_t m = min(kPngItems, n - local);
    for (uint32_t j = 0; j < m; ++j) {
        uint32_t b = f;
        if (c) {
            const uint32_t x = c - 1;
            b = p[x];
            if (f == 1 && x >= 3) b -= p[x - 3];
            if (f == 2 && row) b -= (p - w3)[x];
        }
        fb[local + j] = static_cast<uint8_t>(b);
        if (++c == rowlen) {
            c = 0, ++row, p += w3;
            if (j + 1 < m) f = ftype[row];
        }
    }
}

// This thread's tokens of the tile in fb[0, n)
__device__ __forceinline__ void tokenize(const uint8_t *fb, uint32_t n, uint32_t *ws, uint32_t tok[kPngItems]) {
    uint32_t start[kPngItems], end[kPngItems];
    run_bounds<kPngItems>(fb, n, ws, start, end);
#pragma unroll
    for (uint32_t j = 0; j < kPngItems; ++j) {
        const uint32_t i = threadIdx.x * kPngItems + j;
        tok[j] = i < n ? tile_token(fb[i], i - start[j], end[j] - start[j]) : 0u;
    }
}
// This thread's tokens of the length table ll[0, kPngLens) (2 entries a thread)
__device__ __forceinline__ void tokenize_table(const uint8_t *ll, uint32_t *ws, uint32_t tok[2]) {
    uint32_t start[2], end[2];
    run_bounds<2>(ll, kPngLens, ws, start, end);
#pragma unroll
    for (uint32_t j = 0; j < 2; ++j) {
        const uint32_t i = threadIdx.x * 2 + j;
        tok[j] = i < kPngLens ? table_token(ll[i], i - start[j], end[j] - start[j]) : 0u;
    }
}

__device__ __forceinline__ uint32_t abs_residual(uint32_t v) {
    v &= 255u;
    return v < 128u ? v : 256u - v;
}

// One wave per row: ftype[row] = the filter (0 None, 1 Sub, 2 Up) with the smallest sum
// of |signed residual|, the lower type on a tie; `forced` >= 0 sets it for every row.
// Row 0 has no row above: its Up residuals are None's, so Up never wins there.
__global__ __launch_bounds__(kPngBlock) void rtw_png_filter(const uint8_t *__restrict__ img, uint32_t w3,
                                                            uint32_t height, int forced,
                                                            uint8_t *__restrict__ ftype) {
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, waves = kPngBlock / kWave;
    for (uint32_t row = blockIdx.x * waves + wave; row < height; row += gridDim.x * waves) {
        uint32_t f = static_cast<uint32_t>(forced);
        if (forced < 0) {
            const uint8_t *p = img + static_cast<size_t>(row) * w3;
            uint64_t s[3] = {0, 0, 0};
            for (uint32_t x = lane; x < w3; x += kWave) {
                const uint32_t raw = p[x], left = x >= 3 ? p[x - 3] : 0u, up = row ? (p - w3)[x] : 0u;
                s[0] += abs_residual(raw), s[1] += abs_residual(raw - left), s[2] += abs_residual(raw - up);
            }
#pragma unroll
            for (uint32_t k = 0; k < 3; ++k) {
                uint32_t lo = static_cast<uint32_t>(s[k]), hi = static_cast<uint32_t>(s[k] >> 32);
#pragma unroll
                for (uint32_t m = kWave / 2; m; m >>= 1) {  // 64-bit sum from 32-bit shuffles
                    const uint64_t o = __shfl_xor(lo, m, kWave) | static_cast<uint64_t>(__shfl_xor(hi, m, kWave)) << 32;
                    const uint64_t t = (lo | static_cast<uint64_t>(hi) << 32) + o;
                    lo = static_cast<uint32_t>(t), hi = static_cast<uint32_t>(t >> 32);
                }
                s[k] = lo | static_cast<uint64_t>(hi) << 32;
            }
            f = 0;
            uint64_t best = s[0];
            if (s[1] < best) f = 1, best = s[1];
            if (s[2] < best) f = 2;
        }
        if (lane == 0) ftype[row] = static_cast<uint8_t>(f);
    }
}

// Per tile: recs[t] = {bytes | stored flag, Adler A, Adler B, 0} and, for a tile that
// is not stored, lens[t * 288 ..] = the code lengths of the 286 literal/length symbols
// and of the two distance codes. total = the filtered stream's bytes.
__global__ __launch_bounds__(kPngBlock) void rtw_png_plan(const uint8_t *__restrict__ img,
                                                          const uint8_t *__restrict__ ftype, uint32_t w3,
                                                          uint32_t total, uint32_t n_tiles,
                                                          const PngTables *__restrict__ tabs,
                                                          uint4 *__restrict__ recs, uint8_t *__restrict__ lens) {
    __shared__ __attribute__((aligned(4))) uint8_t fb[kPngTile];
    __shared__ __attribute__((aligned(4))) uint8_t ll[kPngLens];
    __shared__ uint32_t hist[kPngLens], scnt[kPngLens], inner[kPngLens];
    __shared__ uint16_t ssym[kPngLens], lpar[kPngLens], ipar[kPngLens];
    __shared__ uint32_t ws[kPngBlock / kWave], cl_len[19], used, deepest;
    const uint32_t tid = threadIdx.x;
    if (tid < 19) cl_len[tid] = tabs->cl_len[tid];
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint32_t n = min(kPngTile, total - t * kPngTile);
        const bool final_tile = t + 1 == n_tiles;
        for (uint32_t i = tid; i < kPngLens; i += kPngBlock) hist[i] = 0, ll[i] = 0;
        if (tid == 0) deepest = 0;
        load_filtered(img, ftype, w3, t, n, fb);
        __syncthreads();
        uint32_t tok[kPngItems];
        tokenize(fb, n, ws, tok);
        uint32_t a = 0, b = 0, more = 0;
#pragma unroll
        for (uint32_t j = 0; j < kPngItems; ++j) {
            const uint32_t i = tid * kPngItems + j;
            if (tok[j]) atomicAdd(&hist[tok_sym(tok[j])], 1u), more += tok_more(tok[j]);
            if (i < n) a += fb[i], b += (n - i) * fb[i];  // b < 2^32: 255 * 2048 * 2049 / 2
        }
        if (tid == 0) atomicAdd(&hist[256], 1u);
        a = block_reduce<kSum>(a, ws);
        b = block_reduce<kSum>(b, ws);  // its barriers also publish the histogram
        // rank sort of the used symbols by (count, symbol)
        for (uint32_t i = tid; i < kPngLitLen; i += kPngBlock) {
            const uint32_t c = hist[i];
            uint32_t rank = 0, m = 0;
            for (uint32_t j = 0; j < kPngLitLen; ++j) {
                const uint32_t cj = hist[j];
                m += cj != 0;
                rank += cj != 0 && (cj < c || (cj == c && j < i));
            }
            if (c) scnt[rank] = c, ssym[rank] = static_cast<uint16_t>(i);
            if (i == 0) used = m;
        }
        __syncthreads();
        const uint32_t m = used;  // >= 2: a literal and the end of block
        if (tid == 0) {  // two-queue merge: leaves in scnt order, inner nodes in creation order
            uint32_t li = 0, ii = 0;
            for (uint32_t k = 0; k + 1 < m; ++k) {
                uint32_t w = 0;
                for (uint32_t pick = 0; pick < 2; ++pick) {
                    if (li < m && (ii >= k || scnt[li] <= inner[ii])) {
                        w += scnt[li], lpar[li++] = static_cast<uint16_t>(k);
                    } else {
                        w += inner[ii], ipar[ii++] = static_cast<uint16_t>(k);
                    }
                }
                inner[k] = w;
            }
        }
        __syncthreads();
        for (uint32_t r = tid; r < m; r += kPngBlock) {  // a leaf's depth: the walk to the root m - 2
            uint32_t d = 1;
            for (uint32_t p = lpar[r]; p != m - 2; p = ipar[p]) ++d;
            ll[ssym[r]] = static_cast<uint8_t>(d);
            atomicMax(&deepest, d);
        }
        if (tid == 0) ll[kPngLitLen] = ll[kPngLitLen + 1] = 1;  // distance codes 0 and 1: a complete tree
        __syncthreads();
        uint32_t bits = 0;
#pragma unroll
        for (uint32_t j = 0; j < kPngItems; ++j) bits += tok[j] ? ll[tok_sym(tok[j])] : 0u;
        uint32_t tt[2];
        tokenize_table(ll, ws, tt);
#pragma unroll
        for (uint32_t j = 0; j < 2; ++j) bits += tt[j] ? cl_len[tt[j] & 255u] + ((tt[j] >> 8) & 255u) : 0u;
        bits = block_reduce<kSum>(bits + more, ws) + kPrefixBits + ll[256];
        // every tile but the last: 3 bits of an empty stored block, the pad, LEN and NLEN
        const uint32_t coded = final_tile ? (bits + 7) / 8 : (bits + 3 + 7) / 8 + 4;
        const uint32_t stored = rtw::kPngStoredHead + n;
        const bool store = stored <= coded || deepest > 15;  // the depth is < 16 by the tile's size
        if (tid == 0) recs[t] = make_uint4(store ? stored | kStoredFlag : coded, a % kAdlerMod, b % kAdlerMod, 0);
        if (!store && tid < kPngLens / 4)
            reinterpret_cast<uint32_t *>(lens + static_cast<size_t>(t) * kPngLens)[tid] =
                reinterpret_cast<const uint32_t *>(ll)[tid];
        __syncthreads();  // the LDS arrays are reused by the next tile
    }
}

// One workgroup: offsets[t] = kPngHead + the bytes of the tiles before t; ctl = the end
// of the last tile, the Adler-32 of the filtered stream, stored tiles, rows per filter.
// Adler over tiles: a tile of n bytes with partial (a, b) adds n * A + b to B, a to A.
__global__ __launch_bounds__(rtw::kPngScanBlock) void rtw_png_scan(const uint4 *__restrict__ recs, uint32_t n_tiles,
                                                                   uint32_t total,
                                                                   const uint8_t *__restrict__ ftype,
                                                                   uint32_t height, uint64_t *__restrict__ offsets,
                                                                   unsigned long long *__restrict__ ctl) {
    __shared__ uint32_t ws[rtw::kPngScanBlock / kWave];
    const uint32_t tid = threadIdx.x;
    uint64_t carry = kPngHead;
    uint32_t adler_a = 1, adler_b = 0, n_stored = 0;
    for (uint32_t base = 0; base < n_tiles; base += rtw::kPngScanBlock) {
        const uint32_t i = base + tid;
        const uint4 r = i < n_tiles ? recs[i] : make_uint4(0, 0, 0, 0);
        const uint32_t bytes = r.x & ~kStoredFlag, n = i < n_tiles ? min(kPngTile, total - i * kPngTile) : 0u;
        uint32_t all, all_a;
        const uint32_t before = block_excl_sum(bytes, ws, all);
        const uint32_t a_before = block_excl_sum(r.y, ws, all_a);  // < 1024 * 65521
        if (i < n_tiles) offsets[i] = carry + before;
        const uint32_t term = (n * ((adler_a + a_before) % kAdlerMod) + r.z) % kAdlerMod;  // n * A < 2^28
        adler_b = (adler_b + block_reduce<kSum>(term, ws)) % kAdlerMod;
        adler_a = (adler_a + all_a) % kAdlerMod;
        n_stored += block_reduce<kSum>(r.x >> 31, ws);
        carry += all;
    }
    uint32_t rows[3] = {0, 0, 0};
    for (uint32_t y = tid; y < height; y += rtw::kPngScanBlock) {
        const uint32_t f = ftype[y];
        rows[0] += f == 0, rows[1] += f == 1, rows[2] += f == 2;
    }
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) rows[k] = block_reduce<kSum>(rows[k], ws);
    if (tid == 0) {
        ctl[kCtlEnd] = carry, ctl[kCtlAdler] = adler_b << 16 | adler_a, ctl[kCtlStored] = n_stored;
        ctl[kCtlRows] = rows[0], ctl[kCtlRows + 1] = rows[1], ctl[kCtlRows + 2] = rows[2];
    }
}

// value (n bits, n <= 32) into the bit stream of the tile at bit position `pos`; the
// stream's bit k is bit k % 8 of byte k / 8, i.e. bit k % 32 of little-endian word k / 32
__device__ __forceinline__ void put_bits(uint32_t *stage, uint32_t pos, uint32_t value) {
    const uint64_t v = static_cast<uint64_t>(value) << (pos & 31u);
    atomicOr(&stage[pos >> 5], static_cast<uint32_t>(v));
    if (v >> 32) atomicOr(&stage[(pos >> 5) + 1], static_cast<uint32_t>(v >> 32));
}

// Per tile: its deflate block(s) into out[offsets[t], + bytes) and crcs[t] = their
// CRC-32. The stage holds the tile's bytes at the destination's 16-byte phase (stage
// byte i goes to out[off - off % 16 + i]); `out` is 16-byte aligned.
__global__ __launch_bounds__(kPngBlock) void rtw_png_emit(const uint8_t *__restrict__ img,
                                                          const uint8_t *__restrict__ ftype, uint32_t w3,
                                                          uint32_t total, uint32_t n_tiles,
                                                          const PngTables *__restrict__ tabs,
                                                          const uint4 *__restrict__ recs,
                                                          const uint8_t *__restrict__ lens,
                                                          const uint64_t *__restrict__ offsets,
                                                          uint8_t *__restrict__ out, uint32_t *__restrict__ crcs) {
    __shared__ __attribute__((aligned(4))) uint8_t fb[kPngTile];
    __shared__ __attribute__((aligned(4))) uint8_t ll[kPngLens];
    __shared__ __attribute__((aligned(16))) uint32_t stage[kPngStage / 4];
    __shared__ uint32_t code[kPngLens];  // bit-reversed canonical code of a literal/length symbol
    __shared__ uint32_t crc_tab[256], pw[256], cl_code[19], cl_len[19], prefix[3];
    __shared__ uint32_t ws[kPngBlock / kWave], bl_count[16], next_code[16];
    const uint32_t tid = threadIdx.x;
    crc_tab[tid] = tabs->crc[tid], pw[tid] = tabs->pw[tid];
    if (tid < 19) cl_code[tid] = tabs->cl_code[tid], cl_len[tid] = tabs->cl_len[tid];
    if (tid < 3) prefix[tid] = tabs->prefix[tid];
    uint8_t *stage8 = reinterpret_cast<uint8_t *>(stage);
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint32_t n = min(kPngTile, total - t * kPngTile);
        const uint32_t final_tile = t + 1 == n_tiles;
        const uint4 rec = recs[t];
        const uint64_t off = offsets[t];
        const uint32_t bytes = rec.x & ~kStoredFlag, shift = static_cast<uint32_t>(off & 15u), bit0 = shift * 8;
        for (uint32_t i = tid; i < kPngStage / 4; i += kPngBlock) stage[i] = 0;
        if (tid < 16) bl_count[tid] = 0;
        load_filtered(img, ftype, w3, t, n, fb);
        __syncthreads();
        if (rec.x & kStoredFlag) {  // BFINAL, BTYPE = 0 and the pad; LEN; NLEN; the bytes
            if (tid == 0) {
                uint8_t *h = stage8 + shift;
                h[0] = static_cast<uint8_t>(final_tile), h[1] = static_cast<uint8_t>(n), h[2] = static_cast<uint8_t>(n >> 8);
                h[3] = static_cast<uint8_t>(~n), h[4] = static_cast<uint8_t>(~n >> 8);
            }
#pragma unroll
            for (uint32_t j = 0; j < kPngItems; ++j) {
                const uint32_t i = tid * kPngItems + j;
                if (i < n) stage8[shift + rtw::kPngStoredHead + i] = fb[i];
            }
        } else {
            if (tid < kPngLens / 4)
                reinterpret_cast<uint32_t *>(ll)[tid] =
                    reinterpret_cast<const uint32_t *>(lens + static_cast<size_t>(t) * kPngLens)[tid];
            __syncthreads();
            // canonical codes: symbols of one length count up in symbol order
            for (uint32_t i = tid; i < kPngLitLen; i += kPngBlock)
                if (ll[i]) atomicAdd(&bl_count[ll[i]], 1u);
            __syncthreads();
            if (tid == 0) {
                uint32_t c = 0;
                next_code[0] = 0;
                for (uint32_t l = 1; l < 16; ++l) next_code[l] = c = (c + bl_count[l - 1]) << 1;
            }
            __syncthreads();
            for (uint32_t i = tid; i < kPngLitLen; i += kPngBlock) {
                const uint32_t l = ll[i];
                uint32_t same = 0;
                for (uint32_t j = 0; j < i; ++j) same += ll[j] == l;
                code[i] = l ? __brev(next_code[l] + same) >> (32u - l) : 0u;
            }
            __syncthreads();
            // the block header, then the length table
            if (tid < 3) put_bits(stage, bit0 + 32 * tid, prefix[tid] | (tid == 0 ? final_tile : 0u));
            uint32_t tt[2], len2[2], mine = 0, all;
            tokenize_table(ll, ws, tt);
#pragma unroll
            for (uint32_t j = 0; j < 2; ++j) {
                len2[j] = tt[j] ? cl_len[tt[j] & 255u] + ((tt[j] >> 8) & 255u) : 0u;
                mine += len2[j];
            }
            uint32_t pos = bit0 + kPrefixBits + block_excl_sum(mine, ws, all);
#pragma unroll
            for (uint32_t j = 0; j < 2; ++j) {
                if (tt[j]) put_bits(stage, pos, cl_code[tt[j] & 255u] | (tt[j] >> 16 & 255u) << cl_len[tt[j] & 255u]);
                pos += len2[j];
            }
            const uint32_t body = bit0 + kPrefixBits + all;
            // the tokens
            uint32_t tok[kPngItems], len[kPngItems];
            tokenize(fb, n, ws, tok);
            mine = 0;
#pragma unroll
            for (uint32_t j = 0; j < kPngItems; ++j) {
                len[j] = tok[j] ? ll[tok_sym(tok[j])] + tok_more(tok[j]) : 0u;
                mine += len[j];
            }
            pos = body + block_excl_sum(mine, ws, all);
#pragma unroll
            for (uint32_t j = 0; j < kPngItems; ++j) {
                if (tok[j]) {  // the code, the length's extra bits, then the distance code 0
                    const uint32_t s = tok_sym(tok[j]);
                    put_bits(stage, pos, code[s] | ((tok[j] >> kTokExtraShift) & 31u) << ll[s]);
                }
                pos += len[j];
            }
            if (tid == 0) {
                const uint32_t eob = body + all;
                put_bits(stage, eob, code[256]);
                // the empty stored block: 3 zero bits, the pad, LEN = 0, NLEN = 0xffff
                if (!final_tile) put_bits(stage, (eob + ll[256] + 3 + 7) / 8 * 8 + 16, 0xffffu);
            }
        }
        __syncthreads();
        const uint32_t end = shift + bytes;  // stage[shift, end) is the tile
        uint8_t *dst = out + (off - shift);
        for (uint32_t a = tid * 16u; a < end; a += kPngBlock * 16u) {
            if (a >= shift && a + 16u <= end) {
                *reinterpret_cast<uint4 *>(dst + a) = *reinterpret_cast<const uint4 *>(stage8 + a);
            } else {
                const uint32_t lo = a > shift ? a : shift, hi = a + 16u < end ? a + 16u : end;
                for (uint32_t i = lo; i < hi; ++i) dst[i] = stage8[i];
            }
        }
        // the tile's CRC: lane t takes the 9 bytes that end 9 * t before the tile's end
        uint32_t c = 0;
        if (tid * rtw::kPngCrcChunk < bytes) {
            const uint32_t hi = end - tid * rtw::kPngCrcChunk;
            const uint32_t lo = hi - shift > rtw::kPngCrcChunk ? hi - rtw::kPngCrcChunk : shift;
            c = multmodp(pw[tid], crc_bytes(crc_tab, stage8 + lo, hi - lo));
        }
        c = block_reduce<kXor>(c, ws);
        if (tid == 0) crcs[t] = c;
        __syncthreads();  // the stage and the tables of this tile are reused by the next
    }
}

// One workgroup: the CRC-32 of the IDAT chunk (type + data) from its pieces, then the
// bytes around the tiles: signature + IHDR + IDAT length and type + zlib header in
// front, Adler-32 + IDAT CRC + IEND behind.
__global__ __launch_bounds__(rtw::kPngScanBlock) void rtw_png_finish(const uint4 *__restrict__ recs,
                                                                     const uint64_t *__restrict__ offsets,
                                                                     const uint32_t *__restrict__ crcs,
                                                                     uint32_t n_tiles,
                                                                     const PngTables *__restrict__ tabs,
                                                                     unsigned long long *__restrict__ ctl,
                                                                     uint8_t *__restrict__ out, PngHeader hdr) {
    __shared__ uint32_t ws[rtw::kPngScanBlock / kWave], x2n[32], crc_tab[256];
    const uint32_t tid = threadIdx.x;
    if (tid < 32) x2n[tid] = tabs->x2n[tid];
    if (tid < 256) crc_tab[tid] = tabs->crc[tid];
    __syncthreads();
    const uint64_t end = ctl[kCtlEnd];
    const uint32_t adler = static_cast<uint32_t>(ctl[kCtlAdler]);
    const uint8_t trailer[4] = {static_cast<uint8_t>(adler >> 24), static_cast<uint8_t>(adler >> 16),
                                static_cast<uint8_t>(adler >> 8), static_cast<uint8_t>(adler)};
    uint32_t c = 0;
    for (uint32_t i = tid; i < n_tiles; i += rtw::kPngScanBlock)
        c ^= multmodp(xpow8(x2n, end - (offsets[i] + (recs[i].x & ~kStoredFlag)) + 4), crcs[i]);
    if (tid == 0) c ^= multmodp(xpow8(x2n, end - kPngHead + 4), hdr.crc_head) ^ crc_bytes(crc_tab, trailer, 4);
    c = block_reduce<kXor>(c, ws);
    const uint32_t idat_len = static_cast<uint32_t>(end - kPngHead) + 2 + 4;  // zlib header + tiles + Adler-32
    if (tid < kPngHead) out[tid] = tid - 33u < 4u ? static_cast<uint8_t>(idat_len >> (8 * (36 - tid))) : hdr.s[tid];
    if (tid >= kWave && tid < kWave + rtw::kPngTail) {
        const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
        const uint32_t k = tid - kWave;
        out[end + k] = k < 4 ? trailer[k] : k < 8 ? static_cast<uint8_t>(c >> (8 * (7 - k))) : iend[k - 8];
    }
    if (tid == 0) ctl[kCtlCrc] = c;
}

// ------------------------------------------------------------------- host ---
// The fixed code-length code: complete (Kraft sum 1), short codes for what a sparse
// length table is made of. Lengths by symbol 0..18: 0 and 18 take 3 bits, 17 and the
// lengths 3..8 take 4, the rest 5.
constexpr uint8_t kClLen[19] = {3, 5, 5, 4, 4, 4, 4, 4, 4, 5, 5, 5, 5, 5, 5, 5, 5, 4, 3};
constexpr uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

const PngTables &png_tables() {
    static const PngTables tabs = [] {
        PngTables t{};
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = c & 1 ? (c >> 1) ^ kCrcPoly : c >> 1;
            t.crc[i] = c;
        }
        uint32_t p = 1u << 30;  // x^1
        t.x2n[0] = p;
        for (uint32_t n = 1; n < 32; ++n) t.x2n[n] = p = multmodp(p, p);
        for (uint32_t i = 0; i < 256; ++i) t.pw[i] = xpow8(t.x2n, static_cast<uint64_t>(rtw::kPngCrcChunk) * i);
        uint32_t code = 0, kraft = 0;
        for (uint32_t len = 1; len <= 7; ++len, code <<= 1)  // canonical, then bit-reversed
            for (uint32_t s = 0; s < 19; ++s)
                if (kClLen[s] == len) {
                    uint32_t r = 0;
                    for (uint32_t b = 0; b < len; ++b) r |= ((code >> b) & 1u) << (len - 1 - b);
                    t.cl_code[s] = r, t.cl_len[s] = len, ++code, kraft += 128u >> len;
                }
        if (kraft != 128u) throw rtw::Error(RTW_E_ARG, "the code-length code is not complete");
        uint64_t lo = 2u << 1 | 29u << 3 | 1u << 8 | 15u << 13;  // BTYPE, HLIT, HDIST, HCLEN
        uint32_t hi = 0, pos = 17;
        for (uint32_t k = 0; k < 19; ++k, pos += 3) {
            const uint64_t v = kClLen[kClOrder[k]];
            if (pos < 64) lo |= v << pos;
            if (pos + 3 > 64) hi |= static_cast<uint32_t>(pos >= 64 ? v << (pos - 64) : v >> (64 - pos));
        }
        t.prefix[0] = static_cast<uint32_t>(lo), t.prefix[1] = static_cast<uint32_t>(lo >> 32), t.prefix[2] = hi;
        return t;
    }();
    return tabs;
}

// Per-device scratch, grow-only, owned by the library.
struct PngCtx {
    int device = 0;
    std::mutex mu;  // one call at a time per device
    PngTables *d_tabs = nullptr;
    unsigned long long *d_ctl = nullptr, *h_ctl = nullptr;  // h_ctl: pinned
    uint8_t *d_rgb8 = nullptr, *d_ftype = nullptr, *d_lens = nullptr, *d_out = nullptr;
    uint4 *d_recs = nullptr;
    uint64_t *d_offsets = nullptr;
    uint32_t *d_crcs = nullptr;
    size_t rgb8_cap = 0, rows_cap = 0, lens_cap = 0, out_cap = 0, recs_cap = 0, offsets_cap = 0, crcs_cap = 0;
    hipEvent_t ev_done = nullptr, ev[7] = {};
    hipStream_t last_stream = nullptr;
    bool pending = false;  // ev_done was recorded on last_stream
    bool ran = false;
    rtw_png_stats last{};

    ~PngCtx() {
        (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();
        (void)hipFree(d_tabs), (void)hipFree(d_ctl), (void)hipFree(d_rgb8), (void)hipFree(d_ftype);
        (void)hipFree(d_lens), (void)hipFree(d_out), (void)hipFree(d_recs), (void)hipFree(d_offsets);
        (void)hipFree(d_crcs);
        if (h_ctl) (void)hipHostFree(h_ctl);
        if (ev_done) (void)hipEventDestroy(ev_done);
        for (auto e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

std::mutex g_mu;
std::map<int, PngCtx *> g_ctx;

PngCtx *context(int device) {
    std::lock_guard<std::mutex> lock(g_mu);
    auto it = g_ctx.find(device);
    if (it != g_ctx.end()) {
        HIPCHECK(hipSetDevice(device));
        return it->second;
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) throw rtw::Error(RTW_E_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= n) throw rtw::Error(RTW_E_NO_DEVICE, "device index out of range");
    HIPCHECK(hipSetDevice(device));
    auto *c = new PngCtx();
    c->device = device;
    try {
        HIPCHECK(hipMalloc(&c->d_tabs, sizeof(PngTables)));
        HIPCHECK(hipMalloc(&c->d_ctl, kCtlWords * sizeof(unsigned long long)));
        HIPCHECK(hipHostMalloc(&c->h_ctl, kCtlWords * sizeof(unsigned long long)));
        HIPCHECK(hipMemcpy(c->d_tabs, &png_tables(), sizeof(PngTables), hipMemcpyHostToDevice));
        HIPCHECK(hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming));
        for (auto &e : c->ev) HIPCHECK(hipEventCreate(&e));
    } catch (...) {
        delete c;
        throw;
    }
    g_ctx[device] = c;
    return c;
}

template <typename P>
void grow(P *&p, size_t &cap, size_t want) {
    if (want <= cap) return;
    HIPCHECK(hipDeviceSynchronize());  // nothing in flight reads the old buffer
    if (p) HIPCHECK(hipFree(p));
    p = nullptr, cap = 0;
    HIPCHECK(hipMalloc(&p, want * sizeof(P)));
    cap = want;
}

uint32_t be32(uint8_t *p, uint32_t v) {
    p[0] = static_cast<uint8_t>(v >> 24), p[1] = static_cast<uint8_t>(v >> 16);
    p[2] = static_cast<uint8_t>(v >> 8), p[3] = static_cast<uint8_t>(v);
    return v;
}

PngHeader make_header(uint32_t width, uint32_t height) {
    const PngTables &t = png_tables();
    PngHeader h{};
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    std::memcpy(h.s, sig, 8);
    be32(h.s + 8, 13);
    std::memcpy(h.s + 12, "IHDR", 4);
    be32(h.s + 16, width), be32(h.s + 20, height);
    h.s[24] = 8, h.s[25] = 2;  // bit depth, colour type RGB; compression, filter method, interlace: 0
    be32(h.s + 29, crc_bytes(t.crc, h.s + 12, 17));
    std::memcpy(h.s + 37, "IDAT", 4);  // 33..36: the IDAT length, known on the device
    h.s[41] = 0x78, h.s[42] = 0x01;    // zlib: deflate, 32 KiB window, fastest; a multiple of 31
    h.crc_head = crc_bytes(t.crc, h.s + 37, 6);
    return h;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

unsigned grid_of(uint64_t n) { return static_cast<unsigned>(n < 65536 ? n : 65536); }

// src: the frame (is_f32 0/1) or, with from_rgb8, the RGB8 image itself
int64_t encode(int device, const void *src, bool from_rgb8, int is_f32, uint32_t width, uint32_t height, int filter,
               void *hip_stream, char *buf, uint64_t cap) {
    if (!width || !height) throw rtw::Error(RTW_E_EMPTY_IMAGE, "image of zero size");
    if (filter < -1 || filter > 2) throw rtw::Error(RTW_E_ARG, "filter must be -1 (adaptive), 0, 1 or 2");
    const uint64_t rowlen = 1 + 3ull * width;
    if (height > rtw::kPngMaxStream / rowlen) throw rtw::Error(RTW_E_UNSUPPORTED, "image beyond one IDAT chunk");
    const uint64_t total = rowlen * height, n_tiles = (total + kPngTile - 1) / kPngTile;
    const uint64_t worst = total + n_tiles * rtw::kPngStoredHead;
    if (worst + 6 > rtw::kPngMaxStream) throw rtw::Error(RTW_E_UNSUPPORTED, "image beyond one IDAT chunk");
    if (!src) throw rtw::Error(RTW_E_ARG, "null argument");
    DeviceGuard guard;
    PngCtx *c = context(device);
    std::lock_guard<std::mutex> lock(c->mu);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const uint32_t w3 = 3 * width, tiles = static_cast<uint32_t>(n_tiles), n = static_cast<uint32_t>(total);
    if (!from_rgb8) grow(c->d_rgb8, c->rgb8_cap, static_cast<size_t>(w3) * height);
    grow(c->d_ftype, c->rows_cap, height);
    grow(c->d_recs, c->recs_cap, tiles);
    grow(c->d_lens, c->lens_cap, static_cast<size_t>(tiles) * kPngLens);
    grow(c->d_offsets, c->offsets_cap, tiles);
    grow(c->d_crcs, c->crcs_cap, tiles);
    grow(c->d_out, c->out_cap, kPngHead + worst + rtw::kPngTail);
    const uint8_t *img = from_rgb8 ? static_cast<const uint8_t *>(src) : c->d_rgb8;
    if (c->pending && c->last_stream != st) HIPCHECK(hipStreamWaitEvent(st, c->ev_done, 0));
    HIPCHECK(hipEventRecord(c->ev[0], st));
    if (!from_rgb8) {  // asynchronous, on the same stream; a channel above 1 is 255, which is what a PNG wants
        const int rc = rtw_quantise_device(device, src, is_f32, width, height, c->d_rgb8, hip_stream, nullptr);
        if (rc != RTW_OK) throw rtw::Error(rc, rtw::last_error());
    }
    HIPCHECK(hipEventRecord(c->ev[1], st));
    hipLaunchKernelGGL(rtw_png_filter, dim3(grid_of((height + 3) / 4)), dim3(kPngBlock), 0, st, img, w3, height,
                       filter, c->d_ftype);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(c->ev[2], st));
    hipLaunchKernelGGL(rtw_png_plan, dim3(grid_of(tiles)), dim3(kPngBlock), 0, st, img, c->d_ftype, w3, n, tiles,
                       c->d_tabs, c->d_recs, c->d_lens);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(c->ev[3], st));
    hipLaunchKernelGGL(rtw_png_scan, dim3(1), dim3(rtw::kPngScanBlock), 0, st, c->d_recs, tiles, n, c->d_ftype,
                       height, c->d_offsets, c->d_ctl);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(c->ev[4], st));
    hipLaunchKernelGGL(rtw_png_emit, dim3(grid_of(tiles)), dim3(kPngBlock), 0, st, img, c->d_ftype, w3, n, tiles,
                       c->d_tabs, c->d_recs, c->d_lens, c->d_offsets, c->d_out, c->d_crcs);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(c->ev[5], st));
    hipLaunchKernelGGL(rtw_png_finish, dim3(1), dim3(rtw::kPngScanBlock), 0, st, c->d_recs, c->d_offsets, c->d_crcs,
                       tiles, c->d_tabs, c->d_ctl, c->d_out, make_header(width, height));
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(c->ev[6], st));
    HIPCHECK(hipEventRecord(c->ev_done, st));
    c->last_stream = st, c->pending = true;
    HIPCHECK(hipMemcpyAsync(c->h_ctl, c->d_ctl, kCtlWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    c->pending = false;
    float ms[6];
    for (int i = 0; i < 6; ++i) HIPCHECK(hipEventElapsedTime(&ms[i], c->ev[i], c->ev[i + 1]));
    const uint64_t size = c->h_ctl[kCtlEnd] + rtw::kPngTail;
    c->last = rtw_png_stats{ms[0], ms[1], ms[2], ms[3], ms[4], ms[5], 0., n_tiles, c->h_ctl[kCtlStored],
                            c->h_ctl[kCtlRows], c->h_ctl[kCtlRows + 1], c->h_ctl[kCtlRows + 2], total, size};
    c->ran = true;
    if (buf && cap >= size) {
        const auto t0 = std::chrono::steady_clock::now();
        HIPCHECK(hipMemcpy(buf, c->d_out, size, hipMemcpyDeviceToHost));
        c->last.download_ms = ms_since(t0);
    }
    return static_cast<int64_t>(size);
}

}  // namespace

namespace rtw {

void png_shutdown() {
    DeviceGuard guard;
    std::lock_guard<std::mutex> lock(g_mu);
    for (auto &kv : g_ctx) delete kv.second;
    g_ctx.clear();
}

std::string render_png_device(const Camera &cam, const Scene &world, uint32_t samples_sqrt, rtw_u128 seed, bool fast,
                              int device, int filter, rtw_stats *stats) {
    DeviceGuard guard;
    FlatScene flat;
    world.flatten(flat);
    rtw_session *s = nullptr;
    void *d_fb = nullptr;
    auto ok = [](int64_t rc) {
        if (rc < 0) throw Error(static_cast<int>(rc), last_error());
        return rc;
    };
    try {
        ok(rtw_session_create(device, &s));
        ok(rtw_session_set_scene_moving(s, flat.spheres.data(), static_cast<uint32_t>(flat.spheres.size()),
                                        flat.moving ? flat.center1.data() : nullptr,  // null: rtw_session_set_scene
                                        flat.materials.data(), static_cast<uint32_t>(flat.materials.size())));
        const uint64_t n = static_cast<uint64_t>(cam.width()) * cam.height() * 3;
        HIPCHECK(hipSetDevice(device));
        HIPCHECK(hipMalloc(&d_fb, std::max<uint64_t>(n, 1) * (fast ? sizeof(float) : sizeof(double))));
        ok(fast ? rtw_session_render_fast(s, &cam.d, samples_sqrt, seed, nullptr, static_cast<float *>(d_fb), nullptr)
                : rtw_session_render(s, &cam.d, samples_sqrt, seed, nullptr, static_cast<double *>(d_fb), nullptr));
        rtw_stats st{};
        ok(rtw_session_stats(s, &st));  // waits for the render
        if (stats) *stats = st;
        // no tile is larger than its stored form, so the file fits this whatever the image holds
        const uint64_t filtered = (1 + 3ull * cam.width()) * cam.height();
        std::string png(filtered + (filtered / kPngTile + 1) * kPngStoredHead + kPngHead + kPngTail, '\0');
        png.resize(static_cast<size_t>(
            ok(rtw_png_device(device, d_fb, fast, cam.width(), cam.height(), filter, nullptr, &png[0], png.size()))));
        (void)hipFree(d_fb);
        rtw_session_destroy(s);
        return png;
    } catch (...) {
        if (d_fb) (void)hipFree(d_fb);
        rtw_session_destroy(s);
        throw;
    }
}

std::string render_progressive_device(const Camera &cam, const Scene &world, uint32_t samples_sqrt, rtw_u128 seed,
                                      int device, uint32_t passes, const std::string &preview_dir, bool png,
                                      std::vector<float> *frame, std::vector<float> *pass_ms, rtw_stats *stats) {
    DeviceGuard guard;
    FlatScene flat;
    world.flatten(flat);
    rtw_session *s = nullptr;
    void *d_acc = nullptr, *d_fb = nullptr;
    auto ok = [](int64_t rc) {
        if (rc < 0) throw Error(static_cast<int>(rc), last_error());
        return rc;
    };
    try {
        ok(rtw_session_create(device, &s));
        ok(rtw_session_set_scene_moving(s, flat.spheres.data(), static_cast<uint32_t>(flat.spheres.size()),
                                        flat.moving ? flat.center1.data() : nullptr,  // null: rtw_session_set_scene
                                        flat.materials.data(), static_cast<uint32_t>(flat.materials.size())));
        const uint32_t w = cam.width(), h = cam.height();
        const uint64_t n = std::max<uint64_t>(static_cast<uint64_t>(w) * h * 3, 1);
        const uint32_t n_off = samples_sqrt ? samples_sqrt * samples_sqrt : 1;
        passes = std::min(std::max(passes, 1u), n_off);
        HIPCHECK(hipSetDevice(device));
        HIPCHECK(hipMalloc(&d_acc, n * sizeof(unsigned long long)));
        HIPCHECK(hipMalloc(&d_fb, n * sizeof(float)));
        HIPCHECK(hipMemset(d_acc, 0, n * sizeof(unsigned long long)));
        const uint64_t filtered = (1 + 3ull * w) * h;
        std::string file(filtered + (filtered / kPngTile + 1) * kPngStoredHead + kPngHead + kPngTail, '\0');
        const size_t cap = file.size();
        rtw_stats total{};
        uint64_t done = 0;
        for (uint32_t p = 0; p < passes; ++p) {  // pass p: the lattice samples k = p (mod passes)
            const uint32_t k_count = (n_off - p + passes - 1) / passes;
            ok(rtw_session_accumulate_fast(s, &cam.d, samples_sqrt, seed, nullptr, p, passes, k_count,
                                           static_cast<unsigned long long *>(d_acc), nullptr));
            rtw_stats st{};
            ok(rtw_session_stats(s, &st));  // waits for the pass
            done += k_count;
            ok(rtw_resolve_fast(device, static_cast<unsigned long long *>(d_acc), done, w, h,
                                static_cast<float *>(d_fb), nullptr, nullptr));
            if (pass_ms) pass_ms->push_back(st.kernel_ms);
            total.kernel_ms += st.kernel_ms, total.samples += st.samples, total.segments += st.segments;
            total.pixels = st.pixels;
            const bool last = p + 1 == passes;
            if (!preview_dir.empty() || (last && png)) {  // the running mean, as a viewer would see it
                file.resize(cap);
                file.resize(static_cast<size_t>(ok(rtw_png_device(device, d_fb, 1, w, h, -1, nullptr, &file[0], cap))));
            }
            if (!preview_dir.empty()) {
                char name[32];
                std::snprintf(name, sizeof name, "/pass_%04u.png", p);
                FILE *f = std::fopen((preview_dir + name).c_str(), "wb");
                if (!f) throw Error(RTW_E_ARG, "cannot create " + preview_dir + name);
                const bool short_write = std::fwrite(file.data(), 1, file.size(), f) != file.size();
                if (std::fclose(f) != 0 || short_write) throw Error(RTW_E_ARG, "short write");
            }
        }
        if (stats) *stats = total;
        if (!png) {
            HIPCHECK(hipDeviceSynchronize());
            frame->resize(static_cast<size_t>(w) * h * 3);
            HIPCHECK(hipMemcpy(frame->data(), d_fb, frame->size() * sizeof(float), hipMemcpyDeviceToHost));
            file.clear();
        }
        (void)hipFree(d_acc), (void)hipFree(d_fb);
        rtw_session_destroy(s);
        return file;
    } catch (...) {
        if (d_acc) (void)hipFree(d_acc);
        if (d_fb) (void)hipFree(d_fb);
        rtw_session_destroy(s);
        throw;
    }
}

}  // namespace rtw

#define RTW_PNG_GUARD(body)             \
    try {                               \
        return body;                    \
    } catch (const rtw::Error &e) {     \
        rtw::set_error(e.what());       \
        return e.code;                  \
    } catch (const std::exception &e) { \
        rtw::set_error(e.what());       \
        return RTW_E_ARG;               \
    }

extern "C" {

int64_t rtw_png_device(int device, const void *rgb_device, int is_f32, uint32_t width, uint32_t height, int filter,
                       void *hip_stream, char *buf, uint64_t cap) {
    RTW_PNG_GUARD(encode(device, rgb_device, false, is_f32, width, height, filter, hip_stream, buf, cap))
}

int64_t rtw_png_rgb8_device(int device, const uint8_t *rgb8_device, uint32_t width, uint32_t height, int filter,
                            void *hip_stream, char *buf, uint64_t cap) {
    RTW_PNG_GUARD(encode(device, rgb8_device, true, 0, width, height, filter, hip_stream, buf, cap))
}

int rtw_png_device_stats(int device, rtw_png_stats *out) {
    if (!out) return rtw::set_error("null argument"), RTW_E_ARG;
    std::lock_guard<std::mutex> lock(g_mu);
    auto it = g_ctx.find(device);
    if (it == g_ctx.end() || !it->second->ran) return rtw::set_error("no rtw_png_device ran on this device"), RTW_E_ARG;
    std::lock_guard<std::mutex> lock2(it->second->mu);
    *out = it->second->last;
    return RTW_OK;
}

}  // extern "C"

// rtw_ppm.hip -- the output stage on the device: gamma_correct + quantise
// (color.rs:241-247) and Color::wire_full_file's P3 text (color.rs:196-239) for a
// framebuffer that lives in HBM, byte-identical to the host writer (rtw_host.cpp
// format_ppm) for every input. DESIGN.md 3.8.
//
// No pow on the device. For c in (0, 1) the value is the number of thresholds
// T_1..T_255 that c reaches (an 8-step search over bit patterns staged in LDS); inside
// +-64 ulps of a threshold, where the host writer asks the C library's pow, the device
// reads the byte that same pow gave when the host built the table
// (rtw::gamma_device_table). c == 1 is 255, !(c > 0) is 0, and c > 1 is *wide*: stored
// as 255, counted, and the text of such a frame comes from the host writer. (-inf is
// wide too: the C library's pow(-inf, 1/2.2) is +inf, which saturates like +inf.)
//
// Launches, all on the caller's stream, none waiting on another workgroup:
//   rtw_ppm_clear     one wave: zeroes the wide counter
//   rtw_quantise<T>   frame -> RGB8 (one u32 of 4 channels per lane, 256 B per wave)
//                     + the text length of every 4096-channel tile
//   rtw_ppm_scan      one workgroup: exclusive scan of the tile lengths -> 64-bit tile
//                     offsets (from the header's length) and the total
//   rtw_ppm_emit      per tile: block-wide scan of the value lengths, digits and
//                     separators into an LDS stage laid out at the destination's
//                     16-byte phase, then aligned 16-byte stores (bytes at both ends)
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "rtw_capi.h"
#include "rtw_host.h"
#include "rtw_internal.h"
#include "rtw_png.h"
#include "rtw_ppm.h"

namespace {

using rtw::kPpmBlock;
using rtw::kPpmPack;
using rtw::kPpmStage;
using rtw::kPpmSubs;
using rtw::kPpmTile;
constexpr uint32_t kWave = 64;
constexpr uint32_t kWaves = kPpmBlock / kWave;
constexpr uint32_t kNear = static_cast<uint32_t>(rtw::GammaDeviceTable::kNear);
constexpr uint32_t kCtlWide = 0, kCtlTotal = 1, kCtlWords = 2;
static_assert(kPpmPack == 4, "a lane's pack is one u32 of RGB8 and one 16-byte f32 load");

// digits + one separator
__device__ __forceinline__ uint32_t text_len(uint32_t v) { return 2u + (v >= 10u) + (v >= 100u); }

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
    for (uint32_t m = kWave / 2; m; m >>= 1) x += __shfl_xor(x, m, kWave);
    return x;
}
__device__ __forceinline__ uint32_t wave_scan_inclusive(uint32_t x, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < kWave; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, kWave);
        if (lane >= d) x += y;
    }
    return x;
}

__device__ __forceinline__ uint64_t bits_of(double c) { return static_cast<uint64_t>(__double_as_longlong(c)); }
__device__ __forceinline__ uint64_t bits_of(float c) { return bits_of(static_cast<double>(c)); }  // exact widening
// 4 consecutive channels as 16-byte vectors (p is 16-byte aligned)
__device__ __forceinline__ void load_pack(const double *p, uint64_t b[4]) {
    const ulonglong2 lo = reinterpret_cast<const ulonglong2 *>(p)[0];
    const ulonglong2 hi = reinterpret_cast<const ulonglong2 *>(p)[1];
    b[0] = lo.x, b[1] = lo.y, b[2] = hi.x, b[3] = hi.y;
}
__device__ __forceinline__ void load_pack(const float *p, uint64_t b[4]) {
    const float4 f = *reinterpret_cast<const float4 *>(p);
    b[0] = bits_of(f.x), b[1] = bits_of(f.y), b[2] = bits_of(f.z), b[3] = bits_of(f.w);
}

// (c.powf(1/2.2) * 255.0) as u64 of the double with bit pattern b, clipped to 255;
// `wide` counts the inputs whose true value may exceed 255 (c > 1, and +-inf).
__device__ __forceinline__ uint32_t quantise_bits(uint64_t b, const uint64_t *th, const uint8_t *__restrict__ near,
                                                  uint32_t &wide) {
    constexpr uint64_t kOne = 0x3ff0000000000000ull, kInf = 0x7ff0000000000000ull, kSign = 1ull << 63;
    if (b - 1 >= kInf && b != (kSign | kInf)) return 0;  // +0, -0, finite negatives and NaN: pow gives 0 or NaN
    if (b >= kOne) {  // 1 is 255; above it, and -inf (pow(-inf, 1/2.2) = +inf), the value outgrows a byte
        wide += b != kOne;
        return 255;
    }
    uint32_t k = 0;  // largest k with th[k] <= b (th[0] = 0); k + step <= 255 always
#pragma unroll
    for (uint32_t step = 128; step; step >>= 1) k += th[k + step] <= b ? step : 0u;
    const uint64_t above = b - th[k], below = th[k + 1] - b;
    if (above < kNear) return near[k * (2 * kNear) + kNear + static_cast<uint32_t>(above)];
    if (k < 255 && below <= kNear) return near[(k + 1) * (2 * kNear) + kNear - static_cast<uint32_t>(below)];
    return k;
}

__global__ void rtw_ppm_clear(unsigned long long *ctl) {
    if (threadIdx.x < kCtlWords) ctl[threadIdx.x] = 0;
}

// Framebuffer -> RGB8 and counts[t] = text bytes of tile t. Lane `tid` of step `sub`
// owns channels tile*4096 + (sub*256 + tid)*4 .. +3: a wave reads 2 KB (f64) or 1 KB
// (f32) and writes 256 B, all contiguous. vec_in / vec_out: the buffers are 16- /
// 4-byte aligned (else element loads / byte stores; also the tail of the last pack).
template <typename T>
__global__ __launch_bounds__(kPpmBlock) void rtw_quantise(const T *__restrict__ rgb, uint64_t n, uint32_t vec_in,
                                                          uint8_t *__restrict__ rgb8, uint32_t vec_out,
                                                          const uint64_t *__restrict__ g_th,
                                                          const uint8_t *__restrict__ near,
                                                          uint32_t *__restrict__ counts,
                                                          unsigned long long *__restrict__ ctl, uint64_t n_tiles) {
    __shared__ uint64_t th[257];
    __shared__ uint32_t wsum[kWaves];
    const uint32_t tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    for (uint32_t i = tid; i < 257; i += kPpmBlock) th[i] = g_th[i];
    __syncthreads();
    uint32_t wide = 0;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t len = 0;
#pragma unroll
        for (uint32_t sub = 0; sub < kPpmSubs; ++sub) {
            const uint64_t c0 = t * kPpmTile + (sub * kPpmBlock + tid) * kPpmPack;
            if (c0 >= n) continue;
            const uint32_t m = n - c0 < kPpmPack ? static_cast<uint32_t>(n - c0) : kPpmPack;
            uint64_t b[kPpmPack] = {0, 0, 0, 0};
            if (m == kPpmPack && vec_in) {
                load_pack(rgb + c0, b);
            } else {
                for (uint32_t j = 0; j < m; ++j) b[j] = bits_of(rgb[c0 + j]);
            }
            uint32_t packed = 0;
#pragma unroll
            for (uint32_t j = 0; j < kPpmPack; ++j) {
                const uint32_t v = quantise_bits(b[j], th, near, wide);  // b = 0 past the end: 0, not wide
                packed |= v << (8 * j);
                len += j < m ? text_len(v) : 0u;
            }
            if (m == kPpmPack && vec_out) {
                *reinterpret_cast<uint32_t *>(rgb8 + c0) = packed;
            } else {
                for (uint32_t j = 0; j < m; ++j) rgb8[c0 + j] = static_cast<uint8_t>(packed >> (8 * j));
            }
        }
        len = wave_sum(len);
        if (lane == 0) wsum[wave] = len;
        __syncthreads();
        if (tid == 0) {
            uint32_t s = 0;
            for (uint32_t w = 0; w < kWaves; ++w) s += wsum[w];
            counts[t] = s;
        }
        __syncthreads();
    }
    wide = wave_sum(wide);  // one atomic per wave, and only from a wave that has any
    if (lane == 0 && wide) atomicAdd(&ctl[kCtlWide], static_cast<unsigned long long>(wide));
}

// One workgroup: offsets[t] = start + sum of counts[0..t), ctl[total] = start + all.
// 1024 tiles per step (at most 16 MiB of text: 32-bit inside a step, 64-bit carry).
__global__ __launch_bounds__(rtw::kPpmScanBlock) void rtw_ppm_scan(const uint32_t *__restrict__ counts,
                                                                   uint64_t n_tiles, uint64_t start,
                                                                   uint64_t *__restrict__ offsets,
                                                                   unsigned long long *__restrict__ ctl) {
    constexpr uint32_t kScanWaves = rtw::kPpmScanBlock / kWave;
    __shared__ uint32_t wsum[kScanWaves];
    const uint32_t tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    uint64_t carry = start;
    for (uint64_t base = 0; base < n_tiles; base += rtw::kPpmScanBlock) {
        const uint64_t i = base + tid;
        const uint32_t c = i < n_tiles ? counts[i] : 0u;
        const uint32_t x = wave_scan_inclusive(c, lane);
        if (lane == kWave - 1) wsum[wave] = x;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < kScanWaves; ++w) {
            const uint32_t a = wsum[w];
            before += w < wave ? a : 0u;
            all += a;
        }
        if (i < n_tiles) offsets[i] = carry + before + (x - c);
        carry += all;
        __syncthreads();
    }
    if (tid == 0) ctl[kCtlTotal] = carry;
}

struct PpmHeader {
    char s[32];  // "P3\n{W} {H}\n255\n": at most 29 bytes
    uint32_t len;
};

// (global channel index + 1) % row for the first channel of a pack, given the tile's
// first channel modulo row; 32-bit arithmetic whenever the row allows it.
__device__ __forceinline__ uint64_t row_phase(uint64_t tile_rem, uint32_t local, uint64_t row) {
    if (row <= 0x7fffffffull) return (static_cast<uint32_t>(tile_rem) + local + 1u) % static_cast<uint32_t>(row);
    return (tile_rem + local + 1u) % row;
}

// RGB8 -> text, one tile per workgroup iteration. The stage holds the tile's text at
// the destination's 16-byte phase (stage byte i goes to out[off - off % 16 + i]), so
// the copy-out reads and writes aligned 16-byte vectors; the partial vectors at the
// two ends, which neighbouring tiles share, go out as bytes. `out` is 16-byte aligned;
// rgb8 is 4-byte aligned and readable up to the next multiple of 4 past n.
__global__ __launch_bounds__(kPpmBlock) void rtw_ppm_emit(const uint8_t *__restrict__ rgb8, uint64_t n, uint64_t row,
                                                          const uint64_t *__restrict__ offsets, uint64_t n_tiles,
                                                          char *__restrict__ out, PpmHeader hdr) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[kPpmStage];
    __shared__ uint32_t wsum[kPpmSubs][kWaves];
    const uint32_t tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    if (blockIdx.x == 0 && tid < hdr.len) out[tid] = hdr.s[tid];
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t off = offsets[t];
        const uint32_t shift = static_cast<uint32_t>(off & 15u);
        const uint64_t tile_rem = (t * kPpmTile) % row;
        uint32_t run = shift;  // stage position of the next step's first byte
#pragma unroll
        for (uint32_t sub = 0; sub < kPpmSubs; ++sub) {
            const uint32_t local = (sub * kPpmBlock + tid) * kPpmPack;
            const uint64_t c0 = t * kPpmTile + local;
            uint32_t packed = 0, m = 0;
            if (c0 < n) {
                packed = *reinterpret_cast<const uint32_t *>(rgb8 + c0);
                m = n - c0 < kPpmPack ? static_cast<uint32_t>(n - c0) : kPpmPack;
            }
            uint32_t mine = 0;  // in-lane, then across the wave, then across the waves
#pragma unroll
            for (uint32_t j = 0; j < kPpmPack; ++j) mine += j < m ? text_len((packed >> (8 * j)) & 255u) : 0u;
            const uint32_t x = wave_scan_inclusive(mine, lane);
            if (lane == kWave - 1) wsum[sub][wave] = x;
            __syncthreads();
            uint32_t before = 0, all = 0;
#pragma unroll
            for (uint32_t w = 0; w < kWaves; ++w) {
                const uint32_t a = wsum[sub][w];
                before += w < wave ? a : 0u;
                all += a;
            }
            unsigned char *o = stage + run + before + (x - mine);
            run += all;
            if (m) {
                uint64_t r = row_phase(tile_rem, local, row);  // 0: this channel ends an image row
#pragma unroll
                for (uint32_t j = 0; j < kPpmPack; ++j) {
                    if (j < m) {
                        const uint32_t v = (packed >> (8 * j)) & 255u;
                        const uint32_t h = v / 100u, te = (v - h * 100u) / 10u, u = v - h * 100u - te * 10u;
                        if (v >= 100u) *o++ = static_cast<unsigned char>('0' + h);
                        if (v >= 10u) *o++ = static_cast<unsigned char>('0' + te);
                        *o++ = static_cast<unsigned char>('0' + u);
                        *o++ = r == 0 ? '\n' : ' ';  // color.rs:223-233
                        r = r + 1 == row ? 0 : r + 1;
                    }
                }
            }
        }
        __syncthreads();
        const uint32_t end = run;  // stage[shift, end) is the tile's text
        char *dst = out + (off - shift);
        for (uint32_t a = tid * 16u; a < end; a += kPpmBlock * 16u) {
            if (a >= shift && a + 16u <= end) {
                *reinterpret_cast<uint4 *>(dst + a) = *reinterpret_cast<const uint4 *>(stage + a);
            } else {
                const uint32_t lo = a > shift ? a : shift, hi = a + 16u < end ? a + 16u : end;
                for (uint32_t i = lo; i < hi; ++i) dst[i] = static_cast<char>(stage[i]);
            }
        }
        __syncthreads();  // the stage and wsum are reused by the next tile
    }
}

// ------------------------------------------------------------------- host ---
// Per-device scratch, grow-only, owned by the library.
struct PpmCtx {
    int device = 0;
    std::mutex mu;  // one call at a time per device
    uint64_t *d_th = nullptr;
    uint8_t *d_near = nullptr;
    unsigned long long *d_ctl = nullptr, *h_ctl = nullptr;  // h_ctl: pinned
    uint8_t *d_rgb8 = nullptr;
    size_t rgb8_cap = 0;
    uint32_t *d_counts = nullptr;
    uint64_t *d_offsets = nullptr;
    size_t tiles_cap = 0;
    char *d_text = nullptr;
    size_t text_cap = 0;
    hipEvent_t ev_done = nullptr, ev[4] = {};
    hipStream_t last_stream = nullptr;
    bool pending = false;  // ev_done was recorded on last_stream
    rtw_ppm_stats last{};

    ~PpmCtx() {
        (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();
        (void)hipFree(d_th), (void)hipFree(d_near), (void)hipFree(d_ctl), (void)hipFree(d_rgb8);
        (void)hipFree(d_counts), (void)hipFree(d_offsets), (void)hipFree(d_text);
        if (h_ctl) (void)hipHostFree(h_ctl);
        if (ev_done) (void)hipEventDestroy(ev_done);
        for (auto e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

std::mutex g_mu;
std::map<int, PpmCtx *> g_ctx;

PpmCtx *context(int device) {
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
    auto *c = new PpmCtx();
    c->device = device;
    try {
        const rtw::GammaDeviceTable &g = rtw::gamma_device_table();
        HIPCHECK(hipMalloc(&c->d_th, sizeof g.t));
        HIPCHECK(hipMalloc(&c->d_near, sizeof g.near));
        HIPCHECK(hipMalloc(&c->d_ctl, kCtlWords * sizeof(unsigned long long)));
        HIPCHECK(hipHostMalloc(&c->h_ctl, kCtlWords * sizeof(unsigned long long)));
        HIPCHECK(hipMemcpy(c->d_th, g.t, sizeof g.t, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(c->d_near, g.near, sizeof g.near, hipMemcpyHostToDevice));
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
void grow(P *&p, size_t &cap, size_t want, size_t elem) {
    if (want <= cap) return;
    HIPCHECK(hipDeviceSynchronize());  // nothing in flight reads the old buffer
    if (p) HIPCHECK(hipFree(p));
    p = nullptr, cap = 0;
    HIPCHECK(hipMalloc(&p, want * elem));
    cap = want;
}

uint64_t channels_of(uint32_t width, uint32_t height) {
    const uint64_t px = static_cast<uint64_t>(width) * height;
    if (px > rtw::kPpmMaxChannels / 3) throw rtw::Error(RTW_E_UNSUPPORTED, "image beyond 2^40 channels");
    return px * 3;
}

unsigned grid_of(uint64_t n_tiles) { return static_cast<unsigned>(n_tiles < 65536 ? n_tiles : 65536); }

// A call on another stream than the context's previous one waits for it on the device.
void order_after_previous(PpmCtx *c, hipStream_t st) {
    if (c->pending && c->last_stream != st) HIPCHECK(hipStreamWaitEvent(st, c->ev_done, 0));
}
void mark_enqueued(PpmCtx *c, hipStream_t st) {
    HIPCHECK(hipEventRecord(c->ev_done, st));
    c->last_stream = st, c->pending = true;
}

// clear + quantise on st; rgb8 = the caller's buffer, or the context's own
void enqueue_quantise(PpmCtx *c, const void *rgb, bool f32, uint64_t n, uint8_t *rgb8, hipStream_t st) {
    const uint64_t n_tiles = (n + kPpmTile - 1) / kPpmTile;
    size_t cap = c->tiles_cap;
    grow(c->d_counts, cap, n_tiles, sizeof(uint32_t));
    grow(c->d_offsets, c->tiles_cap, n_tiles, sizeof(uint64_t));
    const uint32_t vec_in = reinterpret_cast<uintptr_t>(rgb) % 16 == 0;
    const uint32_t vec_out = reinterpret_cast<uintptr_t>(rgb8) % 4 == 0;
    hipLaunchKernelGGL(rtw_ppm_clear, dim3(1), dim3(kWave), 0, st, c->d_ctl);
    HIPCHECK(hipEventRecord(c->ev[0], st));
    if (f32)
        hipLaunchKernelGGL(rtw_quantise<float>, dim3(grid_of(n_tiles)), dim3(kPpmBlock), 0, st,
                           static_cast<const float *>(rgb), n, vec_in, rgb8, vec_out, c->d_th, c->d_near,
                           c->d_counts, c->d_ctl, n_tiles);
    else
        hipLaunchKernelGGL(rtw_quantise<double>, dim3(grid_of(n_tiles)), dim3(kPpmBlock), 0, st,
                           static_cast<const double *>(rgb), n, vec_in, rgb8, vec_out, c->d_th, c->d_near,
                           c->d_counts, c->d_ctl, n_tiles);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(c->ev[1], st));
}

// the control words after everything enqueued on st: {wide, total}
void read_ctl(PpmCtx *c, hipStream_t st) {
    HIPCHECK(hipMemcpyAsync(c->h_ctl, c->d_ctl, kCtlWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    c->pending = false;
}

uint8_t *own_rgb8(PpmCtx *c, uint64_t n) {
    grow(c->d_rgb8, c->rgb8_cap, (n + 3) / 4 * 4, 1);
    return c->d_rgb8;
}

int quantise(int device, const void *rgb, int is_f32, uint32_t width, uint32_t height, uint8_t *rgb8_device,
             uint8_t *rgb8_host, void *hip_stream, uint64_t *wide) {
    const uint64_t n = channels_of(width, height);
    if (wide) *wide = 0;
    if (!n) return RTW_OK;
    if (!rgb || (!rgb8_device && !rgb8_host)) throw rtw::Error(RTW_E_ARG, "null argument");
    PpmCtx *c = context(device);
    std::lock_guard<std::mutex> lock(c->mu);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    uint8_t *dst = rgb8_device ? rgb8_device : own_rgb8(c, n);
    order_after_previous(c, st);
    enqueue_quantise(c, rgb, is_f32 != 0, n, dst, st);
    if (rgb8_host) HIPCHECK(hipMemcpyAsync(rgb8_host, dst, n, hipMemcpyDeviceToHost, st));
    mark_enqueued(c, st);
    if (wide || rgb8_host) {
        read_ctl(c, st);
        if (wide) *wide = c->h_ctl[kCtlWide];
    }
    return RTW_OK;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int64_t format_device(int device, const void *rgb, int is_f32, uint32_t width, uint32_t height, void *hip_stream,
                      char *buf, uint64_t cap, uint64_t *wide) {
    const uint64_t n = channels_of(width, height);
    if (wide) *wide = 0;
    if (!n) {  // header only, as the host writer; nothing is launched
        const std::string s = rtw::format_ppm(nullptr, width, height);
        if (buf && cap >= s.size()) std::memcpy(buf, s.data(), s.size());
        return static_cast<int64_t>(s.size());
    }
    if (!rgb) throw rtw::Error(RTW_E_ARG, "null argument");
    PpmCtx *c = context(device);
    std::lock_guard<std::mutex> lock(c->mu);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const uint64_t n_tiles = (n + kPpmTile - 1) / kPpmTile;
    PpmHeader hdr{};
    const std::string head = "P3\n" + std::to_string(width) + " " + std::to_string(height) + "\n255\n";
    hdr.len = static_cast<uint32_t>(head.size());
    std::memcpy(hdr.s, head.data(), head.size());
    uint8_t *rgb8 = own_rgb8(c, n);
    grow(c->d_text, c->text_cap, n * rtw::kPpmMaxLen + sizeof hdr.s, 1);  // worst case: "255 " everywhere
    order_after_previous(c, st);
    enqueue_quantise(c, rgb, is_f32 != 0, n, rgb8, st);
    hipLaunchKernelGGL(rtw_ppm_scan, dim3(1), dim3(rtw::kPpmScanBlock), 0, st, c->d_counts, n_tiles,
                       static_cast<uint64_t>(hdr.len), c->d_offsets, c->d_ctl);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(c->ev[2], st));
    // the emit needs the offsets, not the host: it is enqueued before the total comes back
    hipLaunchKernelGGL(rtw_ppm_emit, dim3(grid_of(n_tiles)), dim3(kPpmBlock), 0, st, rgb8, n,
                       static_cast<uint64_t>(width) * 3, c->d_offsets, n_tiles, c->d_text, hdr);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(c->ev[3], st));
    mark_enqueued(c, st);
    read_ctl(c, st);
    float q = 0, s = 0, e = 0;
    HIPCHECK(hipEventElapsedTime(&q, c->ev[0], c->ev[1]));
    HIPCHECK(hipEventElapsedTime(&s, c->ev[1], c->ev[2]));
    HIPCHECK(hipEventElapsedTime(&e, c->ev[2], c->ev[3]));
    const uint64_t n_wide = c->h_ctl[kCtlWide], total = c->h_ctl[kCtlTotal];
    c->last = rtw_ppm_stats{q, s, e, 0., n_tiles, total, n_wide};
    if (wide) *wide = n_wide;
    const auto t0 = std::chrono::steady_clock::now();
    if (n_wide) {  // a value above 255 needs pow: the host writer formats the downloaded frame
        std::vector<double> fb(n);
        if (is_f32) {
            std::vector<float> f(n);
            HIPCHECK(hipMemcpy(f.data(), rgb, n * sizeof(float), hipMemcpyDeviceToHost));
            std::copy(f.begin(), f.end(), fb.begin());
        } else {
            HIPCHECK(hipMemcpy(fb.data(), rgb, n * sizeof(double), hipMemcpyDeviceToHost));
        }
        c->last.download_ms = ms_since(t0);
        return rtw_format_ppm(fb.data(), width, height, buf, cap);
    }
    if (buf && cap >= total) {
        HIPCHECK(hipMemcpy(buf, c->d_text, total, hipMemcpyDeviceToHost));
        c->last.download_ms = ms_since(t0);
    }
    return static_cast<int64_t>(total);
}

}  // namespace

namespace rtw {

void ppm_shutdown() {
    png_shutdown();  // the PNG encoder's contexts (rtw_png.hip) go with this stage's
    DeviceGuard guard;
    std::lock_guard<std::mutex> lock(g_mu);
    for (auto &kv : g_ctx) delete kv.second;
    g_ctx.clear();
}

std::string render_ppm_device(const Camera &cam, const Scene &world, uint32_t samples_sqrt, rtw_u128 seed,
                              bool fast, int device, rtw_stats *stats, uint64_t *wide) {
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
        std::string text(n * kPpmMaxLen + 64, '\0');  // enough unless a channel is wide
        int64_t len = ok(rtw_format_ppm_device(device, d_fb, fast, cam.width(), cam.height(), nullptr, &text[0],
                                               text.size(), wide));
        if (static_cast<uint64_t>(len) > text.size()) {
            text.resize(static_cast<size_t>(len));
            len = ok(rtw_format_ppm_device(device, d_fb, fast, cam.width(), cam.height(), nullptr, &text[0],
                                           text.size(), wide));
        }
        text.resize(static_cast<size_t>(len));
        (void)hipFree(d_fb);
        rtw_session_destroy(s);
        return text;
    } catch (...) {
        if (d_fb) (void)hipFree(d_fb);
        rtw_session_destroy(s);
        throw;
    }
}

}  // namespace rtw

#define RTW_PPM_GUARD(body)               \
    DeviceGuard device_guard_;            \
    try {                                 \
        return body;                      \
    } catch (const rtw::Error &e) {       \
        rtw::set_error(e.what());         \
        return e.code;                    \
    } catch (const std::exception &e) {   \
        rtw::set_error(e.what());         \
        return RTW_E_ARG;                 \
    }

extern "C" {

int rtw_quantise_device(int device, const void *rgb_device, int is_f32, uint32_t width, uint32_t height,
                        uint8_t *rgb8_device, void *hip_stream, uint64_t *wide) {
    RTW_PPM_GUARD(quantise(device, rgb_device, is_f32, width, height, rgb8_device, nullptr, hip_stream, wide))
}

int rtw_quantise_host(int device, const void *rgb_device, int is_f32, uint32_t width, uint32_t height,
                      uint8_t *rgb8_host, void *hip_stream, uint64_t *wide) {
    RTW_PPM_GUARD(quantise(device, rgb_device, is_f32, width, height, nullptr, rgb8_host, hip_stream, wide))
}

int64_t rtw_format_ppm_device(int device, const void *rgb_device, int is_f32, uint32_t width, uint32_t height,
                              void *hip_stream, char *buf, uint64_t cap, uint64_t *wide) {
    RTW_PPM_GUARD(format_device(device, rgb_device, is_f32, width, height, hip_stream, buf, cap, wide))
}

int rtw_ppm_device_stats(int device, rtw_ppm_stats *out) {
    if (!out) return rtw::set_error("null argument"), RTW_E_ARG;
    std::lock_guard<std::mutex> lock(g_mu);
    auto it = g_ctx.find(device);
    if (it == g_ctx.end()) return rtw::set_error("no rtw_format_ppm_device ran on this device"), RTW_E_ARG;
    std::lock_guard<std::mutex> lock2(it->second->mu);
    *out = it->second->last;
    return RTW_OK;
}

}  // extern "C"

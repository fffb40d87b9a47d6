/*
 * rtw_capi.h -- C ABI of the MI355X-native sampling path (librtw.so).
 *
 * Drop-in boundary for NicoElbers/Raytracing_in_a_weekend_rust's per-pixel hot
 * path. The reference has no FFI; its swappable seam is
 *   Camera::threaded_render(cam: &Arc<Camera>, world: &Arc<dyn Hittable>,
 *                           samples_sqrt: usize) -> Result<(), Box<dyn Error>>
 *   (src/raytracing/camera.rs:223-227, called from src/raytracing/mod.rs:123)
 * whose per-ray trait calls (Hittable::hit, hittable.rs:12-14; Material::scatter,
 * materials.rs:7-9) are far too fine-grained to cross a device boundary. So the
 * boundary is at whole-image granularity: the host flattens the scene (spheres +
 * material table) and the derived Camera, and one call renders all pixels.
 * The Rust-side binding a maintainer would add (bindgen + cc) is shown in
 * INTEGRATION.md.
 *
 * All structs are POD and bindgen-clean. All calls are synchronous unless noted,
 * return RTW_OK (0) or a negative RTW_E_* code, never abort, and leave a
 * thread-local message in rtw_last_error(). The caller owns every host buffer for
 * the duration of a call; nothing is retained after return.
 */
#ifndef RTW_CAPI_H
#define RTW_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTW_ABI_VERSION 7

/* ---- error codes ---- */
#define RTW_OK 0
#define RTW_E_ARG (-1)          /* null pointer / bad size / bad shard                 */
#define RTW_E_EMPTY_IMAGE (-2)  /* height or width 0: assert!, camera.rs:267           */
#define RTW_E_FUZZ (-3)         /* Metal fuzz > 1: assert!, materials.rs:47            */
#define RTW_E_MAT_INDEX (-4)    /* sphere refers to a material that does not exist     */
#define RTW_E_HIP (-5)          /* HIP runtime error (message in rtw_last_error)       */
#define RTW_E_UNSUPPORTED (-6)  /* limits of this build (max_depth, table sizes)       */
#define RTW_E_NO_DEVICE (-7)    /* no usable gfx950 device                             */
#define RTW_E_CAPACITY (-8)     /* caller buffer too small (count written anyway)      */

/* ---- plain data ---- */
typedef struct rtw_vec3 { double x, y, z; } rtw_vec3;           /* Vec3/Point3/Color, vec3.rs:9-14 */
typedef struct rtw_u128 { uint64_t lo, hi; } rtw_u128;          /* XorShift state, random.rs:3-6   */

/* Camera after Camera::new (camera.rs:138-221): the derived values the path reads. */
typedef struct rtw_camera {
    uint32_t img_height, img_width, max_depth, _pad0;
    double focal_length, fov;                 /* stored, unused by the path (as in the reference) */
    rtw_vec3 look_from, look_to, vup;
    rtw_vec3 u, v, w;                         /* BasisVecs, camera.rs:96-100                  */
    double viewport_height, viewport_width;
    rtw_vec3 pixel00, pixel_delta_u, pixel_delta_v;
    double defocus_angle, focus_dist;
    rtw_vec3 defocus_disk_u, defocus_disk_v;
} rtw_camera;

/* Material table row: Lambertian{albedo} (materials.rs:11-14), Metal{albedo,fuzz}
 * (39-43), Dielectric{ir} (65-68). Unused fields are ignored. */
enum { RTW_LAMBERTIAN = 0, RTW_METAL = 1, RTW_DIELECTRIC = 2 };
typedef struct rtw_material {
    uint32_t kind, _pad;
    double albedo[3];
    double fuzz;
    double ir;
} rtw_material;

/* Sphere{center, radius, mat} (sphere.rs:11-16); mat indexes the material table. */
typedef struct rtw_sphere {
    double center[3];
    double radius;
    uint32_t mat, _pad;
} rtw_sphere;

/* Rows row_begin + k*row_step for k < n_rows (row-cyclic multi-GPU shards).
 * NULL shard = the whole image. Output row k of a shard is image row
 * row_begin + k*row_step; per-pixel RNG streams depend only on the global pixel
 * index, so any shard reproduces the unsharded pixels bit-for-bit. */
typedef struct rtw_shard { uint32_t row_begin, row_step, n_rows, _pad; } rtw_shard;

typedef struct rtw_stats {
    uint64_t pixels;          /* pixels rendered                                       */
    uint64_t samples;         /* pixels x lattice offsets (samples_sqrt^2, or 1 if 0)  */
    uint64_t segments;        /* traced segments = Scene::hit calls                    */
    uint64_t sphere_tests;    /* segments x n_spheres (brute force, as the reference)  */
    uint64_t wave_iterations; /* sum over waves of the wave's loop trip count          */
    uint64_t exact_tests;     /* f64 sphere tests run after the conservative filter    */
    uint64_t exact_wave_iterations; /* wave-level iterations of the exact-test loop
                                       (fast mode: of the BVH walk loop, diagnostic
                                       builds with -DRTW_FAST_DIAG; else 0)           */
    double kernel_ms;         /* render kernel time, HIP events on the launch stream   */
    uint32_t grid_blocks, block_threads;
    uint64_t node_visits;     /* BVH walk iterations (inner-node or leaf tests), lanes  */
    uint64_t brute_segments;  /* segments the BVH path re-did by brute-force scan      */
    uint32_t accel;           /* 0 brute-force f64, 1 f32-filtered scan, 2 BVH         */
    uint32_t lds_bytes;       /* dynamic LDS per workgroup                             */
    uint64_t parked_pixels;   /* pixels finished by the cooperative second kernel      */
    uint64_t inside_segments; /* segments resolved by the inside cut (rtw_accel.h)     */
    uint64_t trap_segments;   /* segments skipped by the trapped-path fast-forward      */
    /* ABI 5: */
    uint64_t guard_exits;     /* idle waits of the persistent kernel ended by its
                                 no-progress guard ($RTW_SPIN_GUARD_MS, default 100)   */
    uint64_t leftover_pixels; /* parked pixels finished by the follow-up launch (after
                                 guard exits; 0 on an exclusive device)                 */
    /* ABI 6: */
    double main_kernel_ms;    /* the main render kernel alone (persistent / fast kernel),
                                 HIP events around its launch; kernel_ms spans every
                                 launch of the render (seeds, cost order, main, leftover) */
} rtw_stats;

/* ---- library ---- */
const char *rtw_version(void);
/* RTW_ABI_VERSION the library was built with. A client compares it with the
 * RTW_ABI_VERSION of the header it was compiled against before passing any struct
 * (rtw_stats grew in ABI 5 and ABI 6). */
int rtw_abi_version(void);
/* Hash of the library's sources and device flags (profiles/ counter files are
 * stamped with it). */
const char *rtw_build_id(void);
const char *rtw_last_error(void);
int rtw_device_count(int *count);
/* Frees every device resource the library owns: the sessions behind
 * rtw_threaded_render(_fast) and rtw_threaded_render_multi, and the scratch of the
 * device output stage (rtw_quantise_device, rtw_format_ppm_device). Sessions the caller
 * created with rtw_session_create stay the caller's. The next one-shot call
 * re-creates what it needs. Not to be called while another thread renders. */
int rtw_shutdown(void);

/* ---- host mirror of the reference types (bit-exact f64, no FMA) ---- */
/* Camera::new(img_height, img_width, max_depth, focal_length, fov, look_from,
 * look_to, vup, defocus_angle, focus_dist, None) -- camera.rs:138-150.
 * Note the reference's argument order: height before width. */
int rtw_camera_new(uint32_t img_height, uint32_t img_width, uint32_t max_depth,
                   double focal_length, double fov, const rtw_vec3 *look_from,
                   const rtw_vec3 *look_to, const rtw_vec3 *vup, double defocus_angle,
                   double focus_dist, rtw_camera *out);

/* Camera::offset_lattice(dx, dy, num_layers) -- camera.rs:422-450 (the render
 * calls it as (pixel_delta_v, pixel_delta_u, s), camera.rs:243-244). */
int rtw_offset_lattice(const rtw_vec3 *dx, const rtw_vec3 *dy, uint32_t samples_sqrt,
                       rtw_vec3 *out, uint32_t cap, uint32_t *count);

/* Interval::contains_inc / contains_ex -- interval.rs:55-62 */
int rtw_interval_contains_inc(double min, double max, double x);
int rtw_interval_contains_ex(double min, double max, double x);

/* XorShift::next_int / next_01 streams from `seed` (random.rs:33-52). */
int rtw_xorshift_next_int(rtw_u128 seed, uint32_t n, rtw_u128 *out);
int rtw_xorshift_next_01(rtw_u128 seed, uint32_t n, double *out);
/* Children handed to pixels first_pixel .. first_pixel+count-1 by the row-major
 * copy_reset chain of threaded_render (camera.rs:255, 269-272; random.rs:61-69),
 * computed by GF(2) jump-ahead (no serial walk). */
int rtw_seed_children(rtw_u128 seed, uint64_t first_pixel, uint64_t count, rtw_u128 *out);

/* Built-in scenes (raytracing/mod.rs). name: "complex" (54-126, the book's final
 * scene; `seed` replaces the wall-clock XorShift::default at mod.rs:67),
 * "simple" (129-173), "threads" (176-202), "super_simple" (205-238), and
 * "three_lambertian" (BASELINE config 1: simple() with the dielectric dropped and
 * the metal sphere made Lambertian). img_height/img_width/max_depth override the
 * builder's hard-coded values when non-zero. Writes up to `cap` spheres and
 * materials; *n_spheres / *n_mats receive the full counts. "bouncing" is RTW_E_ARG here:
 * that scene moves, and rtw_scene_bouncing returns it with its second centres. */
int rtw_scene_builtin(const char *name, rtw_u128 seed, uint32_t img_height, uint32_t img_width,
                      uint32_t max_depth, rtw_camera *cam, rtw_sphere *spheres,
                      rtw_material *mats, uint32_t cap, uint32_t *n_spheres, uint32_t *n_mats);

/* Color::wire_full_file (color.rs:196-247) on an H*W*3 f64 framebuffer (row 0 =
 * top). rtw_format_ppm returns the byte count (writes only if buf && cap
 * suffice); rtw_write_ppm writes the file. */
int64_t rtw_format_ppm(const double *rgb, uint32_t width, uint32_t height, char *buf,
                       uint64_t cap);
int rtw_write_ppm(const char *path, const double *rgb, uint32_t width, uint32_t height);

/* ---- the hot path ---- */
/* Camera::threaded_render equivalent: renders `shard` (NULL = all rows) of the
 * scene into out_rgb (host, n_rows*W*3 f64, row-major), on device 0 (or
 * $RTW_DEVICE). Per-pixel RNG: child p of `seed` (random.rs:61-69). Validation
 * mirrors the reference's asserts. stats may be NULL. */
int rtw_threaded_render(const rtw_camera *cam, const rtw_sphere *spheres, uint32_t n_spheres,
                        const rtw_material *mats, uint32_t n_mats, uint32_t samples_sqrt,
                        rtw_u128 seed, const rtw_shard *shard, double *out_rgb,
                        rtw_stats *stats);

/* Camera::threaded_render on several GPUs of this node (camera.rs:223-227; the
 * reference's pool takes every core, camera.rs:253 -- this takes every listed GPU).
 * `devices` holds n_devices device indices; NULL or 0 = every visible device. An
 * index may repeat: every entry gets its own session, stream and host thread.
 * Rows are dealt cyclically -- image row r goes to entry r % n_devices (sky rows
 * are cheap, ground rows are not) -- and each entry copies its rows straight into
 * their places in out_rgb (host, H*W*3 f64) with one strided device-to-host copy:
 * the gather needs no collective because the result is a host buffer. Pixels and
 * their RNG streams depend only on the global pixel index, so the image is
 * bit-identical to rtw_threaded_render's. stats (nullable): counters summed over
 * the entries, kernel_ms = the slowest entry's render. */
int rtw_threaded_render_multi(const rtw_camera *cam, const rtw_sphere *spheres, uint32_t n_spheres,
                              const rtw_material *mats, uint32_t n_mats, uint32_t samples_sqrt,
                              rtw_u128 seed, const int *devices, uint32_t n_devices, double *out_rgb,
                              rtw_stats *stats);

/* rtw_threaded_render_multi in f32 fast mode (ABI 7; see rtw_session_render_fast):
 * same device list, row dealing and strided gather into out_rgb (host, H*W*3 f32). */
int rtw_threaded_render_multi_fast(const rtw_camera *cam, const rtw_sphere *spheres,
                                   uint32_t n_spheres, const rtw_material *mats, uint32_t n_mats,
                                   uint32_t samples_sqrt, rtw_u128 seed, const int *devices,
                                   uint32_t n_devices, float *out_rgb, rtw_stats *stats);

/* rtw_threaded_render in f32 fast mode (see rtw_session_render_fast). */
int rtw_threaded_render_fast(const rtw_camera *cam, const rtw_sphere *spheres, uint32_t n_spheres,
                             const rtw_material *mats, uint32_t n_mats, uint32_t samples_sqrt,
                             rtw_u128 seed, const rtw_shard *shard, float *out_rgb,
                             rtw_stats *stats);

/* Device-resident sessions: scene uploaded once, renders enqueued on a caller
 * stream into a caller device buffer (inputs already in HBM when timing). */
typedef struct rtw_session rtw_session;
int rtw_session_create(int device, rtw_session **out);
int rtw_session_destroy(rtw_session *s);
int rtw_session_set_scene(rtw_session *s, const rtw_sphere *spheres, uint32_t n_spheres,
                          const rtw_material *mats, uint32_t n_mats);
/* Asynchronous: enqueues the render of `shard` on `hip_stream` (a hipStream_t;
 * NULL = HIP's null stream, as everywhere in HIP) writing out_rgb_device (device
 * pointer, n_rows*W*3 f64).
 * Concurrency: all renders of one session share its device buffers, so at most
 * one runs at a time -- a render enqueued on a different stream than the
 * session's previous render waits for it (hipStreamWaitEvent). Use one session
 * per concurrent render. Completeness (one write per pixel) is checked on the
 * device after EVERY render and latched: rtw_session_stats fails if any render
 * since its previous call was incomplete, even if later renders were enqueued
 * before it was called.
 * Residency: the persistent kernel (one workgroup per CU) is fastest with the
 * device to itself, but never depends on all of its workgroups being resident at
 * once: waves that wait for parked pixels leave after $RTW_SPIN_GUARD_MS (default
 * 100) without progress anywhere, and a follow-up launch finishes any parked
 * pixel they left (rtw_stats.guard_exits / leftover_pixels). */
int rtw_session_render(rtw_session *s, const rtw_camera *cam, uint32_t samples_sqrt,
                       rtw_u128 seed, const rtw_shard *shard, double *out_rgb_device,
                       void *hip_stream);
/* f32 fast mode (SURVEY 8(c) "Fast mode"; the ABI sketch's rtw_mode FAST_F32):
 * the same camera, scene, materials and depth rule in f32, with independent
 * xoroshiro64** streams per (pixel, lattice sample) instead of the reference's
 * per-pixel XorShift chain. NOT bit-exact: statistically equal to the parity
 * render (tests/test_gpu_fast.py). Deterministic, and any shard reproduces the
 * unsharded pixels bit-for-bit. Output: n_rows*W*3 f32. Per-sample colours are
 * clamped to [0, min(65536, 2^31 / spp)] (NaN -> 0). */
int rtw_session_render_fast(rtw_session *s, const rtw_camera *cam, uint32_t samples_sqrt,
                            rtw_u128 seed, const rtw_shard *shard, float *out_rgb_device,
                            void *hip_stream);
/* Waits for the session's last render and reports its statistics. */
int rtw_session_stats(rtw_session *s, rtw_stats *out);
/* Diagnostic (not part of the reference surface): per-pixel records of the last
 * render when it ran with RTW_DIAG=1 in the environment -- for pixel p of the
 * shard (row-major), out[2p] = traced segments of the pixel in the one-lane
 * kernel, out[2p+1] = low 32 bits of the 100 MHz device real-time clock when
 * the pixel completed (0 = never ran); out[2 x pixels] = the clock at the persistent
 * launch's start. Returns RTW_E_CAPACITY if cap < 2 x pixels + 4. */
int rtw_session_diag(rtw_session *s, uint32_t *out, uint64_t cap);

/* ---- device-resident multi-GPU renders (ABI 7) ----
 * A group is the node-level Camera::threaded_render (camera.rs:223-352; the
 * reference's pool takes every core, camera.rs:253 -- a group takes every listed
 * GPU) with the image left in HBM: one session per entry of `devices` (NULL or 0
 * entries = every visible device; an index may repeat), image row r rendered by
 * entry r % n, the row tiles gathered on the root device (entry 0) and
 * un-permuted there into the caller's device buffer. The gather is one ncclGather
 * over xGMI (RCCL communicators from ncclCommInitAll) when the entries are
 * distinct GPUs, device-to-device copies otherwise (a repeated device, or
 * RTW_GROUP_COPY_GATHER). If RCCL cannot be loaded or its communicators fail to
 * come up, the group falls back to the copy gather (peer access over xGMI) and
 * says why (rtw_group_info.fallback, rtw_group_note); only RTW_GROUP_RCCL_ALWAYS
 * makes that an error. Renders are blocking: on return the image is complete in
 * out_rgb_device. The root device's first write to out_rgb_device is ordered
 * after the work already queued on that device's null stream (or on the caller's
 * stream: rtw_group_render_on). Every rtw_group_*
 * call restores the caller's current HIP device. Bit-identical to a one-device
 * render. */
typedef struct rtw_group rtw_group;
#define RTW_GROUP_COPY_GATHER 1u /* flags: never RCCL, gather by device copies          */
#define RTW_GROUP_RCCL_ALWAYS 2u /* flags: RCCL gather even for a one-entry group; no
                                    fallback: an RCCL failure is an error (tests)      */
#define RTW_GROUP_RCCL_TRY 4u    /* flags: RCCL gather for a one-entry group too, with
                                    the fallback (tests of the fallback on one GPU)    */
enum { RTW_GATHER_NONE = 0, RTW_GATHER_COPY = 1, RTW_GATHER_RCCL = 2 };
enum { RTW_FALLBACK_NONE = 0, RTW_FALLBACK_NO_RCCL = 1, RTW_FALLBACK_COMM_INIT = 2 };
typedef struct rtw_group_info {
    uint32_t n_entries;     /* entries that rendered rows in the last render (min(n, H)) */
    uint32_t gather;        /* RTW_GATHER_* the last render used                        */
    double wall_ms;         /* host wall time of the last rtw_group_render(_fast)       */
    double render_ms_max;   /* slowest entry's render (HIP events on its own stream)     */
    double root_gather_ms;  /* root stream, from its own tile rendered to the image
                               complete: waiting for the other entries + gather +
                               un-permute                                               */
    uint32_t fast;          /* the last render was f32 fast mode                        */
    uint32_t fallback;      /* RTW_FALLBACK_*: why the group gathers by copies although
                               its entries are distinct GPUs (RCCL unloadable, or
                               ncclCommInitAll failed); text in rtw_group_note       */
} rtw_group_info;
int rtw_group_create(const int *devices, uint32_t n_devices, uint32_t flags, rtw_group **out);
int rtw_group_destroy(rtw_group *g);
int rtw_group_set_scene(rtw_group *g, const rtw_sphere *spheres, uint32_t n_spheres,
                        const rtw_material *mats, uint32_t n_mats);
/* out_rgb_device: H*W*3 f64 on the root device. */
int rtw_group_render(rtw_group *g, const rtw_camera *cam, uint32_t samples_sqrt, rtw_u128 seed,
                     double *out_rgb_device);
/* f32 fast mode; out_rgb_device: H*W*3 f32 on the root device. */
int rtw_group_render_fast(rtw_group *g, const rtw_camera *cam, uint32_t samples_sqrt,
                          rtw_u128 seed, float *out_rgb_device);
/* The same, ordered after the work queued on caller_stream (a hipStream_t of the root
 * device; NULL = its null stream, what rtw_group_render does) instead of the null
 * stream: a caller inside torch.cuda.stream(s), or on a per-thread default stream,
 * passes that stream. Still blocking. */
int rtw_group_render_on(rtw_group *g, const rtw_camera *cam, uint32_t samples_sqrt, rtw_u128 seed,
                        double *out_rgb_device, void *caller_stream);
int rtw_group_render_fast_on(rtw_group *g, const rtw_camera *cam, uint32_t samples_sqrt,
                             rtw_u128 seed, float *out_rgb_device, void *caller_stream);
/* Last render: total (counters summed, times the slowest entry's; nullable),
 * per_entry[0..n_entries) (nullable; RTW_E_CAPACITY if cap < n_entries) and info
 * (nullable). */
int rtw_group_stats(rtw_group *g, rtw_stats *total, rtw_stats *per_entry, uint32_t cap,
                    rtw_group_info *info);
/* Why the group fell back from RCCL to the copy gather ("" if it did not). Owned by
 * the group, valid until rtw_group_destroy. */
const char *rtw_group_note(rtw_group *g);
/* 1 if RCCL (librccl.so.1 with ncclCommInitAll/ncclGather) can be loaded, else 0 with
 * the reason in why[0..cap) (nullable). Needs no GPU. */
int rtw_rccl_available(char *why, size_t cap);

/* ---- the output stage on the device ----
 * gamma_correct + quantise + Color::wire_full_file (color.rs:196-247) for a frame that
 * lives in HBM (rtw_session_render(_fast), rtw_group_render(_fast)): hand-written HIP,
 * no pow on the device. rgb_device: height*width*3 f64 (is_f32 = 0) or f32 (is_f32 != 0:
 * widened to f64 exactly, then the same path) on `device`; `height` is the number of
 * rows in the buffer, so a shard's tile works as well as a whole frame. The RGB8 image
 * and the text are byte-identical to rtw_format_ppm's for EVERY input. A channel > 1
 * (+inf included; also -inf, whose pow is +inf) is *wide*: its text can exceed "255"
 * and needs pow, so it is stored as 255 in the RGB8 image and counted. Scratch lives in a per-device context the
 * library owns (rtw_shutdown frees it); calls on one device are serialised, and ordered
 * on the device across streams. Every call restores the caller's current HIP device.
 * hip_stream: a hipStream_t of `device` (NULL = the null stream). */

/* RGB8 (height*width*3 bytes, row-major) into rgb8_device. wide == NULL: asynchronous,
 * enqueued on hip_stream. wide != NULL: waits, and *wide = the number of wide channels.
 * A zero-sized image launches nothing. */
int rtw_quantise_device(int device, const void *rgb_device, int is_f32, uint32_t width,
                        uint32_t height, uint8_t *rgb8_device, void *hip_stream, uint64_t *wide);
/* The same into a host buffer (blocking): quantised into the context's own RGB8 image
 * and downloaded, 1/8 of the f64 frame's bytes. wide is nullable. */
int rtw_quantise_host(int device, const void *rgb_device, int is_f32, uint32_t width,
                      uint32_t height, uint8_t *rgb8_host, void *hip_stream, uint64_t *wide);
/* rtw_format_ppm for a device frame (blocking). Returns the byte count; writes buf
 * (host) only if buf != NULL and cap suffices. Three kernels on hip_stream (quantise +
 * per-tile text sizes, scan of the tile offsets, text emit), then the text alone is
 * downloaded. If any channel is wide the frame is downloaded instead and the host
 * writer's bytes are returned: identical to rtw_format_ppm either way. *wide (nullable)
 * = the number of wide channels, i.e. which path ran. A zero-sized image behaves as
 * rtw_format_ppm does and launches nothing. */
int64_t rtw_format_ppm_device(int device, const void *rgb_device, int is_f32, uint32_t width,
                              uint32_t height, void *hip_stream, char *buf, uint64_t cap,
                              uint64_t *wide);
/* The last rtw_format_ppm_device of `device`: kernel times from HIP events on its
 * stream, and what it produced. */
typedef struct rtw_ppm_stats {
    double quantise_ms, scan_ms, emit_ms; /* the three kernels                          */
    double download_ms;                   /* host wall time of the text (or, on the wide
                                             fallback, framebuffer) download            */
    uint64_t tiles;                       /* text tiles (4096 channels each)            */
    uint64_t text_bytes;                  /* bytes of the device text, header included  */
    uint64_t wide;                        /* wide channels (non-zero: host fallback ran) */
} rtw_ppm_stats;
int rtw_ppm_device_stats(int device, rtw_ppm_stats *out);

/* ---- PNG on the device ----
 * A complete PNG file (signature, IHDR: 8-bit RGB, no interlace; one IDAT holding one
 * zlib stream; IEND) made in HBM by hand-written HIP and downloaded once. The filtered
 * stream, height * (1 + 3 * width) bytes, is cut into tiles of 2048 bytes; a workgroup
 * encodes a tile as a dynamic-Huffman deflate block of literals and distance-1 matches
 * (zlib's Z_RLE), or stored when that is not larger. filter: 0 None, 1 Sub, 2 Up for every
 * row, or -1: per row the one with the smallest sum of |signed residual| (ties to the
 * lower type). Both calls block, return the file's byte count and write buf (host) only
 * if buf != NULL and cap suffices; height * (1 + 3 * width) * (1 + 5 / 2048) + 100 always
 * does. Errors, found before any device work: width or height 0 is RTW_E_EMPTY_IMAGE,
 * a filter outside -1..2 RTW_E_ARG, an image whose stream could pass 2^31 - 1 bytes
 * (one IDAT) RTW_E_UNSUPPORTED. Scratch, serialisation, stream order and the caller's
 * device are handled as for the stage above; rtw_shutdown frees the scratch. */

/* From a frame (height*width*3 f64, or f32 with is_f32 != 0) on `device`: quantised on
 * hip_stream by rtw_quantise_device into the encoder's own RGB8 image (a channel above
 * 1 is 255, as an 8-bit PNG wants), then encoded. */
int64_t rtw_png_device(int device, const void *rgb_device, int is_f32, uint32_t width,
                       uint32_t height, int filter, void *hip_stream, char *buf, uint64_t cap);
/* From an RGB8 image (height*width*3 bytes, row-major) on `device`. */
int64_t rtw_png_rgb8_device(int device, const uint8_t *rgb8_device, uint32_t width,
                            uint32_t height, int filter, void *hip_stream, char *buf,
                            uint64_t cap);
/* The last PNG call of `device`: kernel times from HIP events on its stream, and what
 * it produced. */
typedef struct rtw_png_stats {
    double quantise_ms, filter_ms, plan_ms, scan_ms, emit_ms, finish_ms; /* the stages   */
    double download_ms;      /* host wall time of the file's download (0: buf not written) */
    uint64_t tiles;          /* deflate tiles (2048 filtered bytes each)                  */
    uint64_t stored_tiles;   /* of them, emitted as stored blocks                         */
    uint64_t rows_none, rows_sub, rows_up; /* rows per filter type                        */
    uint64_t filtered_bytes; /* height * (1 + 3 * width)                                  */
    uint64_t png_bytes;      /* the file                                                  */
} rtw_png_stats;
int rtw_png_device_stats(int device, rtw_png_stats *out);

/* ---- progressive fast mode (ABI 7 additions) ----
 * A fast-mode pixel is an exact, order-free sum of 32.32 fixed-point sample colours, each a
 * function of (seed, global pixel, lattice sample k) alone. So the lattice may be traced in
 * passes into a buffer of sums that the caller keeps, and looked at after every pass. */

/* Adds lattice samples k_first + i*k_step (i < k_count) of every pixel of `shard` to
 * acc_device: n_rows*W*3 u64 on the session's device, caller-owned, row-major like the
 * f32 frame. Each channel is the sum of the samples' colours in 32.32 fixed point.
 * Same camera, scene, seed mix, per-(pixel,k) streams, lattice positions and clamp
 * (cmax from samples_sqrt^2, not from k_count) as rtw_session_render_fast. So accumulating
 * every k of the lattice exactly once, in any split and order, into a zeroed buffer
 * gives the sums of the one-shot render.
 * Range: the buffer holds any number of accumulations while 2^32 * (sum of colours) < 2^63
 * per channel; scenes whose colours stay in [0, 1] (the reference's) have room for 2^31
 * samples per pixel.
 * Asynchronous on hip_stream. Ordering, latch and rtw_session_stats as for
 * rtw_session_render_fast (pixels, samples = pixels*k_count, segments, kernel_ms ...).
 * Errors, found before any device work: a null acc_device, k_step == 0 with k_count > 1,
 * or k_first + (k_count-1)*k_step >= samples_sqrt^2 (1 when samples_sqrt is 0) is
 * RTW_E_ARG; rtw_session_render_fast's own checks apply. k_count == 0 launches nothing
 * and succeeds. */
int rtw_session_accumulate_fast(rtw_session *s, const rtw_camera *cam, uint32_t samples_sqrt,
                                rtw_u128 seed, const rtw_shard *shard, uint32_t k_first,
                                uint32_t k_step, uint32_t k_count,
                                unsigned long long *acc_device, void *hip_stream);

/* Resolves sums to images. Asynchronous on hip_stream. Either output may be NULL, not both.
 * out_rgb_device: height*width*3 f32 = (float)((double)acc * 2^-32 / (double)n_samples),
 *   the one-shot kernel's own expression, so a completed lattice is bit-identical to
 *   rtw_session_render_fast. The gamma-corrected outputs need nothing new:
 *   rtw_quantise_device, rtw_format_ppm_device and rtw_png_device take this frame.
 * preview_rgba8_device: height*width*4 bytes (4-byte aligned) as the reference's
 *   Application::draw fills its window frame: per channel ((double)mean_f32 * 255.) as u8
 *   (Rust's saturating cast: truncation, NaN and negatives 0, above 255 -> 255), linear, no
 *   gamma, A = 0xFF. One aligned 32-bit store per pixel.
 * Errors: a null acc_device, both outputs null or n_samples == 0 is RTW_E_ARG; width or
 * height 0 is RTW_E_EMPTY_IMAGE. */
int rtw_resolve_fast(int device, const unsigned long long *acc_device, uint64_t n_samples,
                     uint32_t width, uint32_t height, float *out_rgb_device,
                     uint8_t *preview_rgba8_device, void *hip_stream);

/* ---- adaptive fast mode (ABI 7 additions) ----
 * Samples go only to the pixels whose mean is still noisy. Let N = max(1, samples_sqrt^2);
 * the adaptive calls need N <= 65535 (a larger N is RTW_E_UNSUPPORTED). Three caller-owned
 * device buffers extend acc (rows*W*3 u64); pixel indices are shard-local and row-major:
 *   counts  rows*W u32: the samples each pixel has so far.
 *   mom     rows*W*2 u64. A finished sample with fixed-point channels R, G, B (what is added
 *           to acc) has q = min((R+G+B) >> 16, 2^24 - 1), its luminance sum in units of
 *           2^-16; mom[p][0] += q, mom[p][1] += q*q. With n <= 65535 samples neither sum
 *           overflows: q^2 < 2^48.
 * Sample order. A pixel's i-th sample (i = 0, 1, ...) is lattice sample k = (i*k_mul) mod N
 *   (the product in 64 bits), gcd(k_mul, N) = 1: every k once, and the first few spread over
 *   the lattice instead of coming from its first rows.
 * Convergence. Exact unsigned 128-bit integer arithmetic (mod 2^128). With n = counts[p],
 *   A = mom[p][0], B = mom[p][1], T = tol_q16 <= 65535 (the relative standard error of the
 *   mean, units of 2^-16) and F = floor_q16 <= 2^24 (a luminance floor in q units, so dark
 *   pixels do not sample forever):
 *     D = n*B - A*A,  E = (A + n*F) >> 8,
 *     conv(p) <=> T > 0 and n >= 2 and (D << 16) <= T*T*(n-1)*E*E,
 *   which is sigma_mean <= t*(mu + f) with both sides scaled by n^2 (n-1) 2^16. Bit budget
 *   for sums the accumulate built: A < 2^40, B < 2^64, 0 <= D < 2^80 so D*2^16 < 2^96;
 *   E < 2^33, so the right side < 2^32 * 2^16 * 2^66 = 2^114. T = 0: never converged.
 * Selection. u(p) = n < N and not conv(p); listed(p) = n < N and u holds for p or for any of
 *   its up-to-8 neighbours inside the rows*W buffer (the usual guard against a pixel that
 *   stops early by luck). A list holds the listed pixels in ascending order. */

/* The default k_mul: 1 for N <= 2, else the integer coprime to N nearest to
 * N*(sqrt(5)-1)/2 (evaluated in IEEE double), ties to the lower. Host only, needs no GPU. */
uint32_t rtw_lattice_stride(uint32_t N);

/* For every pixel p of the list, with n0 = counts[p]: traces ordinals [n0, min(n0+m, N)),
 * adds their colours to acc and q, q*q to mom, and stores the new count. A pixel outside
 * the list is not touched. list_device: n_list u32 on the device, each pixel at most once;
 * n_list_device: the length, a u32 on the device (the host need not know it). A NULL
 * list_device means every pixel of the shard (n_list_device is then ignored). Every m in
 * 1..65535 is served by one kernel built for m >= 16; below that it keeps 8*m lanes of a
 * wave busy. Asynchronous on hip_stream. Ordering, latch and rtw_session_stats as for
 * rtw_session_accumulate_fast; samples is the number actually traced.
 * Errors, found before any device work: rtw_session_accumulate_fast's checks; a null acc,
 * mom or counts, m == 0 or m > 65535, or gcd(k_mul, N) != 1 is RTW_E_ARG. */
int rtw_session_accumulate_fast_list(rtw_session *s, const rtw_camera *cam, uint32_t samples_sqrt,
                                     rtw_u128 seed, const rtw_shard *shard,
                                     const uint32_t *list_device, const uint32_t *n_list_device,
                                     uint32_t m, uint32_t k_mul, unsigned long long *acc_device,
                                     unsigned long long *mom_device, uint32_t *counts_device,
                                     void *hip_stream);

/* Writes the listed pixels (ascending) to list_out_device (room for rows*width u32) and their
 * number to n_list_out_device (one u32). Asynchronous on hip_stream: two passes over one bit
 * per pixel, a scan and an emit. Scratch lives in a per-device context the library owns
 * (rtw_shutdown frees it); calls on one device are serialised and ordered on the device
 * across streams, and the caller's current HIP device is restored.
 * Errors: a null pointer, a mom_device that is not 16-byte aligned (a pixel's two sums are
 * read as one), N == 0, tol_q16 > 65535 or floor_q16 > 2^24 is RTW_E_ARG;
 * N > 65535 RTW_E_UNSUPPORTED; width or rows 0 RTW_E_EMPTY_IMAGE. */
int rtw_adaptive_select(int device, const uint32_t *counts_device,
                        const unsigned long long *mom_device, uint32_t width, uint32_t rows,
                        uint32_t N, uint32_t tol_q16, uint32_t floor_q16,
                        uint32_t *list_out_device, uint32_t *n_list_out_device, void *hip_stream);

/* rtw_resolve_fast with the divisor read per pixel from counts_device: the same expression,
 * (float)((double)acc * 2^-32 / (double)n), and the same RGBA8 rule. A pixel with count 0
 * resolves to 0. Errors as rtw_resolve_fast. */
int rtw_resolve_fast_counts(int device, const unsigned long long *acc_device,
                            const uint32_t *counts_device, uint32_t width, uint32_t rows,
                            float *out_rgb_device, uint8_t *preview_rgba8_device,
                            void *hip_stream);

typedef struct rtw_adaptive_info {
    uint32_t rounds;      /* accumulate launches, the first (every pixel) included        */
    uint32_t selects;     /* selections run                                               */
    uint64_t samples;     /* samples traced = the sum of the final counts                 */
    uint64_t pixels_full; /* pixels that reached N                                        */
    double kernel_ms;     /* the accumulate kernels, summed, from HIP events              */
    double select_ms;     /* the selections, summed, from HIP events                      */
} rtw_adaptive_info;

/* The driver; it blocks. On buffers the session owns: zero acc, mom and counts; one round over
 * every pixel with m = min(max(min_samples, 2), N); then select, read the 4-byte list length
 * and, while it is not 0, accumulate the list with m = batch; at the end resolve by counts
 * into out_rgb_device (rows*W*3 f32) and copy the counts to counts_out_device (rows*W u32,
 * nullable). k_mul = rtw_lattice_stride(N). With tol_q16 = 0 every pixel reaches N and the
 * frame is rtw_session_render_fast's bit for bit. info is nullable.
 * Errors: rtw_session_accumulate_fast_list's and rtw_adaptive_select's; batch == 0 or
 * batch > 65535 is RTW_E_ARG. */
int rtw_session_render_fast_adaptive(rtw_session *s, const rtw_camera *cam, uint32_t samples_sqrt,
                                     rtw_u128 seed, const rtw_shard *shard, uint32_t tol_q16,
                                     uint32_t floor_q16, uint32_t min_samples, uint32_t batch,
                                     float *out_rgb_device, uint32_t *counts_out_device,
                                     void *hip_stream, rtw_adaptive_info *info);

/* ---- denoised fast mode (ABI 7 additions) ----
 * An edge-stopping a-trous filter of a fast-mode frame, driven by the frame's own variance
 * (the adaptive buffers' counts and luminance moments) and by first-hit guides. The scene is
 * spheres of one albedo each: on a sphere the normal determines the position, so there is no
 * depth term, and equal tags mean equal albedo, so nothing is demodulated. What is seen through
 * glass has no guide; Dielectric first hits pass through unfiltered by default. */

/* Guides: one 16-byte record (nx, ny, nz, bits(tag)) per pixel of `shard` into guides_device
 * (n_rows*W float4, 16-byte aligned, row-major like the frame), from the pixel-centre ray:
 * rtw_session_render_fast's primary ray at samples_sqrt = 0, its origin look_from whatever
 * defocus_angle is; nothing random. A hit (the fast-mode closest hit, t_min = 0.01 |d|) writes
 * the shading normal (p - c)/r flipped to face the ray and tag = kind << 30 | sphere index
 * (kinds RTW_LAMBERTIAN, RTW_METAL, RTW_DIELECTRIC = 0, 1, 2). A miss writes the unit ray
 * direction, of which the sky's colour is a function, and tag = 0xffffffff.
 * Asynchronous on hip_stream. Ordering, latch and errors as rtw_session_accumulate_fast;
 * rtw_session_stats reports pixels, samples = segments = pixels and kernel_ms. A null
 * guides_device is RTW_E_ARG; a scene of 2^30 spheres or more RTW_E_UNSUPPORTED. */
int rtw_session_guides_fast(rtw_session *s, const rtw_camera *cam, const rtw_shard *shard,
                            float *guides_device, void *hip_stream);

typedef struct rtw_denoise_params {
    uint32_t levels;       /* 0..8 a-trous levels, step 2^l; 0 = resolve only. default 5 */
    uint32_t normal_log2;  /* 0..8: normal weight = max(0, n_p.n_q)^(2^normal_log2). default 5 */
    uint32_t filter_mask;  /* bit kind (0,1,2) and bit 3 = sky: first-hit kinds that are filtered;
                              other pixels pass through every level unchanged. default 0xB */
    float    sigma_l;      /* luminance stop, in standard deviations of the mean. default 4 */
} rtw_denoise_params;

/* The filter over rows*width pixels, in f32. A pixel's kind is tag >> 30 (3: sky).
 * Prepare. C0[p] = (r, g, b, v) with n = counts[p], A = mom[p][0], B = mom[p][1]:
 *   r, g, b = (float)((double)acc * 2^-32 / (double)n), rtw_resolve_fast_counts's expression;
 *   0 at n = 0. L = (r + g) + b. v, the variance of the mean of L:
 *   n >= 2: D = n*B - A*A in unsigned 128-bit arithmetic (mod 2^128),
 *           v = (float)((double)D * 2^-32 / ((double)n * (double)n * (double)(n-1))),
 *           (double)D the nearest double; n = 1: v = L*L; n = 0: v = 0.
 * Level l = 0 .. levels-1, C -> C'. Step t = 2^l, taps q = p + t*(i, j), i, j in -2..2, those
 *   outside the buffer skipped; h = (1/16, 1/4, 3/8, 1/4, 1/16).
 *   g_p = the (1,2,1)x(1,2,1) weighted mean of C[.].v over the in-buffer pixels p + t*(-1..1)^2,
 *         normalised by the weights present;
 *   w(p,q) = h_i h_j [tag_q == tag_p] max(0, n_p.n_q)^(2^normal_log2)
 *            exp(-|L_p - L_q| / (sigma_l sqrt(g_p) + 1e-6)),
 *         the power by normal_log2 squarings, the exponential as exp2 of the scaled argument;
 *   C'[p].rgb = sum_q w C[q].rgb / sum_q w,  C'[p].v = sum_q w^2 C[q].v / (sum_q w)^2.
 *   The centre tap goes through the same formula; the taps are summed j outer, i inner, so the
 *   result is deterministic. A pixel whose kind's bit is not set in filter_mask: C'[p] = C[p].
 * The last level (prepare when levels = 0) writes out_rgb_device (rows*width*3 f32), v to
 * out_var_device (rows*width f32, nullable) and the RGBA8 preview of rtw_resolve_fast
 * (nullable, 4-byte aligned). levels = 0 is rtw_resolve_fast_counts bit for bit. The frame
 * feeds rtw_quantise_device, rtw_format_ppm_device and rtw_png_device like every fast frame.
 * Asynchronous on hip_stream. Two float4 planes live in a per-device context the library owns
 * (rtw_shutdown frees it); calls on one device are serialised and ordered on the device across
 * streams, and the caller's current HIP device is restored. params NULL: the defaults.
 * Errors, found before any device work: a null acc, counts, mom, guides or out_rgb; guides or
 * mom not 16-byte aligned; levels > 8; normal_log2 > 8; filter_mask > 15; a negative or
 * non-finite sigma_l: RTW_E_ARG. width or rows 0: RTW_E_EMPTY_IMAGE. 2^31 pixels or more:
 * RTW_E_UNSUPPORTED. */
int rtw_denoise_fast(int device, const unsigned long long *acc_device, const uint32_t *counts_device,
                     const unsigned long long *mom_device, const float *guides_device,
                     uint32_t width, uint32_t rows, const rtw_denoise_params *params,
                     float *out_rgb_device, float *out_var_device, uint8_t *preview_rgba8_device,
                     void *hip_stream);

/* rtw_session_render_fast_adaptive's rounds (the same buffers, loop and info; tol_q16 = 0 is the
 * uniform frame), then rtw_session_guides_fast and rtw_denoise_fast instead of the resolve by
 * counts, into out_rgb_device and out_var_device (nullable). It blocks. *denoise_ms (nullable):
 * the filter's kernels, from HIP events; the guides' time is rtw_session_stats' kernel_ms.
 * Errors: both calls' and the adaptive driver's; a shard with row_step != 1 is RTW_E_ARG (the
 * filter needs a pixel's neighbours in the buffer). */
int rtw_session_render_fast_denoised(rtw_session *s, const rtw_camera *cam, uint32_t samples_sqrt,
                                     rtw_u128 seed, const rtw_shard *shard, uint32_t tol_q16,
                                     uint32_t floor_q16, uint32_t min_samples, uint32_t batch,
                                     const rtw_denoise_params *params, float *out_rgb_device,
                                     float *out_var_device, uint32_t *counts_out_device,
                                     void *hip_stream, rtw_adaptive_info *info, double *denoise_ms);

/* ---- motion blur in fast mode (ABI 7 additions) ----
 * Spheres that move in a straight line while the shutter is open, t in [0, 1). Every sample has
 * a time of its own, and a sample at time t sees static spheres at c(t). f64 parity mode has no
 * motion (the reference has none to be bit-exact against). */

/* rtw_session_set_scene with a second centre per sphere. center1: n_spheres*3 doubles; sphere i is
 * at spheres[i].center at time 0 and at center1[i] at time 1, its radius constant. With
 * c0 = f32(center0) and v = f32(center1 - center0) (the difference in f64, then rounded), the
 * sphere at time t is c(t) = fmaf(t, v, c0) per component, the same expression in the closest
 * hit and in the shading normal. A sphere moves if any component of its v is not zero. If
 * center1 is NULL or no sphere moves, the call is rtw_session_set_scene: the same tables, kernels
 * and bits. A later rtw_session_set_scene makes the session static again. Limits and validation
 * are rtw_session_set_scene's.
 * On a moving scene rtw_session_render_fast, rtw_session_accumulate_fast,
 * rtw_session_accumulate_fast_list and rtw_session_render_fast_adaptive work as on a static one,
 * and every split of the lattice still adds up to rtw_session_render_fast's frame bit for bit.
 * rtw_session_render, rtw_session_guides_fast and rtw_session_render_fast_denoised return
 * RTW_E_UNSUPPORTED before any device work (a first hit at one instant is no guide for a blurred
 * pixel). Groups and the rtw_threaded_render* one-shots take static scenes only. */
int rtw_session_set_scene_moving(rtw_session *s, const rtw_sphere *spheres, uint32_t n_spheres,
                                 const double *center1, const rtw_material *mats, uint32_t n_mats);

/* The time of lattice sample k (k < N) of a pixel, in units of 2^-24: t = T24 * 2^-24, exact in
 * f32. A pure function of its arguments that takes nothing from the sample's random stream. With
 * N = max(1, samples_sqrt^2) (an N of 0 is read as 1), g = rtw_lattice_stride(N), global_pixel =
 * y*W + x of the whole image and seed_mix = seed.lo ^ seed.hi*0x9e3779b97f4a7c15 (mod 2^64):
 *   j    = (k*g) mod N, the product in 64 bits: a bijection, and (k, j) is a rank-1 lattice, so
 *          time does not line up with the sub-pixel row as k/N would;
 *   base = floor((2j + 1) * 2^23 / N);
 *   H    = fmix64(fmix64(seed_mix ^ global_pixel*0x9e3779b97f4a7c15) + 2^32) >> 40, fmix64
 *          SplitMix64's finaliser; the inner hash is the streams' own, whose k < 2^32 never
 *          reaches the added constant;
 *   T24  = (base + H) mod 2^24.
 * A pixel's N times fall one in each stratum [i/N, (i+1)/N) of [0, 1) rotated by H, so
 * neighbouring pixels show noise and not N shared ghost images. Host only, needs no GPU. */
uint32_t rtw_fast_sample_time(rtw_u128 seed, uint64_t global_pixel, uint32_t k, uint32_t N);

/* The "bouncing" scene: rtw_scene_builtin("complex", seed, ...) bit for bit (camera, spheres,
 * materials, order), and for every sphere a row of center1 (cap*3 doubles, nullable):
 * center1 = center0 + (0, 0.5*u, 0) for each small (radius 0.2) Lambertian sphere, center0 for
 * every other. The u are next_01 draws, in sphere order, of an XorShift of their own whose state
 * is seed with 0x626f756e63696e67 ("bouncing") xored into its low half; complex's own draws are
 * not disturbed. Counts, capacity and errors as rtw_scene_builtin. */
int rtw_scene_bouncing(rtw_u128 seed, uint32_t img_height, uint32_t img_width, uint32_t max_depth,
                       rtw_camera *cam, rtw_sphere *spheres, double *center1, rtw_material *mats,
                       uint32_t cap, uint32_t *n_spheres, uint32_t *n_mats);

/* ---- device probes (tests) ---- */
/* Device jump-ahead seeds (the kernel's own code path) for a pixel range. */
int rtw_probe_device_seeds(int device, rtw_u128 seed, uint64_t first_pixel, uint64_t count,
                           rtw_u128 *out);
/* Device f64 sqrt(a) and a/b, to check correct rounding against the host. */
int rtw_probe_f64_ops(int device, const double *a, const double *b, uint64_t n,
                      double *out_sqrt, double *out_div);

#ifdef __cplusplus
}
#endif
#endif /* RTW_CAPI_H */

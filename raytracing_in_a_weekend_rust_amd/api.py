"""Python mirror of the reference's trait surface for the sampling path, over the
C ABI (include/rtw_capi.h). Same names and argument order as the reference:

    cam = Camera.new(height, width, max_depth, focal_length, fov,
                     look_from, look_to, vup, defocus_angle, focus_dist)   # camera.rs:138-150
    world = SceneBuilder(); world.add(Sphere.new_world_obj(x, y, z, r, mat)); world.build()
    Camera.threaded_render(cam, world, samples_sqrt, seed=...)             # camera.rs:223-227

Rendering always runs the HIP megakernel in librtw.so; there is no Python/CPU
render path. Errors the reference raises by assert!/panic come back as RtwError
with the matching RTW_E_* code.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np

from . import _capi as capi
from ._capi import RtwError, check, lib

DEFAULT_SEED = 1764892800000  # ms since epoch at 2025-12-05T00:00Z (XorShift::default stand-in)


def _v(t) -> capi.Vec3:
    return capi.Vec3(float(t[0]), float(t[1]), float(t[2]))


# ---------------------------------------------------------------- materials --
class Material:
    def flatten(self) -> capi.Material:
        raise NotImplementedError


@dataclass(eq=False)
class Lambertian(Material):  # materials.rs:11-20
    albedo: tuple

    def flatten(self):
        m = capi.Material()
        m.kind = capi.LAMBERTIAN
        m.albedo[:] = [float(a) for a in self.albedo]
        return m


@dataclass(eq=False)
class Metal(Material):  # materials.rs:39-50
    albedo: tuple
    fuzz: float

    def __post_init__(self):
        if not self.fuzz <= 1.0:  # assert!(fuzz <= 1.), materials.rs:47
            raise RtwError(-3, "Fuzz cannot be more than 1")

    def flatten(self):
        m = capi.Material()
        m.kind = capi.METAL
        m.albedo[:] = [float(a) for a in self.albedo]
        m.fuzz = float(self.fuzz)
        return m


@dataclass(eq=False)
class Dielectric(Material):  # materials.rs:65-73
    ir: float

    def flatten(self):
        m = capi.Material()
        m.kind = capi.DIELECTRIC
        m.ir = float(self.ir)
        return m


# ---------------------------------------------------------------- hittables --
@dataclass(eq=False)
class Sphere:  # sphere.rs:11-37
    center: tuple
    radius: float
    mat: Material
    center1: tuple | None = None  # at time 1 (fast-mode motion blur); None: the sphere stands still

    @staticmethod
    def new_world_obj(x, y, z, radius, mat) -> "Sphere":
        return Sphere((x, y, z), radius, mat)

    @staticmethod
    def new_moving_world_obj(c0, c1, radius, mat) -> "Sphere":
        """The book's moving sphere: at c0 when the shutter opens (t = 0), at c1 when it closes."""
        return Sphere(tuple(c0), radius, mat, tuple(c1))


@dataclass(eq=False)
class Scene:  # hittable.rs:119-143
    objects: list = field(default_factory=list)

    def flatten(self):
        """Sphere and material tables in insertion order; materials are shared
        by identity like Arc<dyn Material>. An empty scene flattens to zero
        spheres (the reference's `Empty`, hittable.rs:98-106)."""
        mats, index = [], {}
        sph = (capi.Sphere * max(1, len(self.objects)))()
        for i, o in enumerate(self.objects):
            if id(o.mat) not in index:
                index[id(o.mat)] = len(mats)
                mats.append(o.mat.flatten())
            s = sph[i]
            s.center[:] = [float(c) for c in o.center]
            s.radius = float(o.radius)
            s.mat = index[id(o.mat)]
        mt = (capi.Material * max(1, len(mats)))(*mats)
        return sph, len(self.objects), mt, len(mats)

    def flatten_moving(self):
        """flatten() with center1 after the spheres' count, as Session.set_scene_moving takes it:
        3 doubles per sphere, its centre at time 1 (its centre for a sphere that stands still)."""
        sph, n, mt, nm = self.flatten()
        c1 = (C.c_double * max(3, 3 * n))()
        for i, o in enumerate(self.objects):
            c1[3 * i:3 * i + 3] = [float(c) for c in (o.center if o.center1 is None else o.center1)]
        return sph, n, c1, mt, nm


class SceneBuilder:  # hittable.rs:86-117
    def __init__(self):
        self.objects = []

    def add(self, obj):
        self.objects.append(obj)

    def build(self) -> Scene:
        return Scene(list(self.objects))


# ------------------------------------------------------------------- camera --
class Camera:
    """Wraps rtw_camera (the derived values of Camera::new)."""

    def __init__(self, raw: capi.Camera):
        self.raw = raw

    @staticmethod
    def new(img_height, img_width, max_depth, focal_length, fov, look_from, look_to, vup,
            defocus_angle, focus_dist) -> "Camera":
        raw = capi.Camera()
        check(lib.rtw_camera_new(img_height, img_width, max_depth, focal_length, fov,
                                 C.byref(_v(look_from)), C.byref(_v(look_to)), C.byref(_v(vup)),
                                 defocus_angle, focus_dist, C.byref(raw)))
        return Camera(raw)

    def width(self):
        return self.raw.img_width

    def height(self):
        return self.raw.img_height

    @staticmethod
    def offset_lattice(dx, dy, num_layers):  # camera.rs:422-450
        n = C.c_uint32()
        lib.rtw_offset_lattice(C.byref(_v(dx)), C.byref(_v(dy)), num_layers, None, 0, C.byref(n))
        out = (capi.Vec3 * max(1, n.value))()
        check(lib.rtw_offset_lattice(C.byref(_v(dx)), C.byref(_v(dy)), num_layers, out, n.value,
                                     C.byref(n)))
        return [out[i].tup() for i in range(n.value)]

    @staticmethod
    def threaded_render(cam: "Camera", world: Scene, samples_sqrt: int, seed: int = DEFAULT_SEED,
                        ppm_path: str | None = "img.ppm", shard=None, devices=None):
        """camera.rs:223-352 on the GPUs of this node: the reference's pool takes every
        core (camera.rs:253), this takes every visible GPU (`devices` None) or the
        listed ones (rtw_threaded_render_multi). `shard` renders only those rows, on
        one device (rtw_threaded_render). Returns (framebuffer HxWx3 f64, stats)."""
        sph, ns, mt, nm = world.flatten()
        if shard is not None:
            fb, st = render_flat(cam.raw, sph, ns, mt, nm, samples_sqrt, seed, shard)
        else:
            fb, st = render_flat_multi(cam.raw, sph, ns, mt, nm, samples_sqrt, seed, devices)
        if ppm_path is not None and shard is None:
            write_ppm(ppm_path, fb)
        return fb, st


# ---------------------------------------------------------------- functions --
def builtin_scene(name: str, seed: int = DEFAULT_SEED, height=0, width=0, max_depth=0):
    """Flattened built-in scene (raytracing/mod.rs): (Camera, spheres, n, mats, nm)."""
    ns, nm = C.c_uint32(), C.c_uint32()
    cam = capi.Camera()
    rc = lib.rtw_scene_builtin(name.encode(), capi.U128.of(seed), height, width, max_depth,
                               C.byref(cam), None, None, 0, C.byref(ns), C.byref(nm))
    if rc not in (0, -8):
        check(rc)
    cap = max(ns.value, nm.value, 1)
    sph, mt = (capi.Sphere * cap)(), (capi.Material * cap)()
    check(lib.rtw_scene_builtin(name.encode(), capi.U128.of(seed), height, width, max_depth,
                                C.byref(cam), sph, mt, cap, C.byref(ns), C.byref(nm)))
    return Camera(cam), sph, ns.value, mt, nm.value


def bouncing_scene(seed: int = DEFAULT_SEED, height=0, width=0, max_depth=0):
    """rtw_scene_bouncing: builtin_scene("complex") with its small Lambertian spheres moving up
    while the shutter is open: (Camera, spheres, n, center1, mats, nm) for Session.set_scene_moving."""
    ns, nm = C.c_uint32(), C.c_uint32()
    cam, args = capi.Camera(), (capi.U128.of(seed), height, width, max_depth)
    rc = lib.rtw_scene_bouncing(*args, C.byref(cam), None, None, None, 0, C.byref(ns), C.byref(nm))
    if rc not in (0, -8):
        check(rc)
    cap = max(ns.value, nm.value, 1)
    sph, mt, c1 = (capi.Sphere * cap)(), (capi.Material * cap)(), (C.c_double * (3 * cap))()
    check(lib.rtw_scene_bouncing(*args, C.byref(cam), sph, c1, mt, cap, C.byref(ns), C.byref(nm)))
    return Camera(cam), sph, ns.value, c1, mt, nm.value


def fast_sample_time(seed: int, global_pixel: int, k: int, n: int) -> int:
    """rtw_fast_sample_time: the time of lattice sample k of n of a pixel on a moving scene, in
    units of 2^-24 (no GPU needed)."""
    return lib.rtw_fast_sample_time(capi.U128.of(seed), global_pixel, k, n)


def _shard(shard):
    if shard is None:
        return None
    if isinstance(shard, capi.Shard):
        return shard
    b, step, n = shard
    return capi.Shard(b, step, n, 0)


def render_flat(cam: capi.Camera, sph, n_sph, mats, n_mats, samples_sqrt, seed=DEFAULT_SEED,
                shard=None):
    """rtw_threaded_render: host buffers in, (n_rows x W x 3 f64, Stats) out."""
    sh = _shard(shard)
    n_rows = cam.img_height if sh is None else sh.n_rows
    fb = np.zeros((n_rows, cam.img_width, 3), dtype=np.float64)
    st = capi.Stats()
    check(lib.rtw_threaded_render(C.byref(cam), sph, n_sph, mats, n_mats, samples_sqrt,
                                  capi.U128.of(seed), C.byref(sh) if sh is not None else None,
                                  fb.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st)))
    return fb, st


def render_flat_multi(cam: capi.Camera, sph, n_sph, mats, n_mats, samples_sqrt, seed=DEFAULT_SEED,
                      devices=None):
    """rtw_threaded_render_multi: the whole image over a list of GPUs (None = every
    visible device; an index may repeat), rows dealt cyclically, gathered by strided
    device-to-host copies into one host framebuffer. Returns (H x W x 3 f64, Stats)."""
    fb = np.zeros((cam.img_height, cam.img_width, 3), dtype=np.float64)
    st = capi.Stats()
    devs = list(devices or [])
    arr = (C.c_int * max(1, len(devs)))(*devs)
    check(lib.rtw_threaded_render_multi(C.byref(cam), sph, n_sph, mats, n_mats, samples_sqrt,
                                        capi.U128.of(seed), arr if devs else None, len(devs),
                                        fb.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st)))
    return fb, st


def render_flat_multi_fast(cam: capi.Camera, sph, n_sph, mats, n_mats, samples_sqrt,
                           seed=DEFAULT_SEED, devices=None):
    """rtw_threaded_render_multi_fast: render_flat_multi in f32 fast mode."""
    fb = np.zeros((cam.img_height, cam.img_width, 3), dtype=np.float32)
    st = capi.Stats()
    devs = list(devices or [])
    arr = (C.c_int * max(1, len(devs)))(*devs)
    check(lib.rtw_threaded_render_multi_fast(C.byref(cam), sph, n_sph, mats, n_mats, samples_sqrt,
                                             capi.U128.of(seed), arr if devs else None, len(devs),
                                             fb.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st)))
    return fb, st


def shutdown():
    """rtw_shutdown: frees the device resources of the one-shot and multi-GPU calls."""
    check(lib.rtw_shutdown())


def build_id() -> str:
    return lib.rtw_build_id().decode()


def render_flat_fast(cam: capi.Camera, sph, n_sph, mats, n_mats, samples_sqrt, seed=DEFAULT_SEED,
                     shard=None):
    """rtw_threaded_render_fast (f32 fast mode, statistical parity): host buffers in,
    (n_rows x W x 3 f32, Stats) out."""
    sh = _shard(shard)
    n_rows = cam.img_height if sh is None else sh.n_rows
    fb = np.zeros((n_rows, cam.img_width, 3), dtype=np.float32)
    st = capi.Stats()
    check(lib.rtw_threaded_render_fast(C.byref(cam), sph, n_sph, mats, n_mats, samples_sqrt,
                                       capi.U128.of(seed), C.byref(sh) if sh is not None else None,
                                       fb.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st)))
    return fb, st


def format_ppm(fb: np.ndarray) -> bytes:
    fb = np.ascontiguousarray(fb, dtype=np.float64)
    h, w = fb.shape[0], fb.shape[1]
    p = fb.ctypes.data_as(C.POINTER(C.c_double))
    # one formatting pass in the common case: values in [0, 1] give <= 4 bytes a
    # channel; the size query + second call only when a brighter image overflows
    cap = 12 * w * h + h + 64
    buf = C.create_string_buffer(cap)
    n = check(lib.rtw_format_ppm(p, w, h, buf, cap))
    if n > cap:
        buf = C.create_string_buffer(n)
        check(lib.rtw_format_ppm(p, w, h, buf, n))
    return C.string_at(buf, n)


def write_ppm(path: str, fb: np.ndarray):
    fb = np.ascontiguousarray(fb, dtype=np.float64)
    check(lib.rtw_write_ppm(path.encode(), fb.ctypes.data_as(C.POINTER(C.c_double)),
                            fb.shape[1], fb.shape[0]))


def quantise_device(ptr: int, shape, fast: bool = False, device: int = 0, stream: int = 0,
                    out_dev_ptr: int | None = None):
    """rtw_quantise_device / rtw_quantise_host: the frame at device pointer `ptr` (shape
    (rows, W[, 3]); f64, or f32 with fast=True) as the 8-bit image the PPM's numbers
    are, made on the GPU. Returns (rows x W x 3 uint8 numpy array, wide), or, when
    `out_dev_ptr` (a device buffer of rows*W*3 bytes) is given, writes there and returns
    (None, wide). wide = channels above 1, stored as 255. Blocking. `stream`: a
    hipStream_t handle of `device` (0 = the null stream)."""
    h, w = int(shape[0]), int(shape[1])
    wide = C.c_uint64()
    if out_dev_ptr is not None:
        check(lib.rtw_quantise_device(device, C.c_void_p(ptr), int(fast), w, h, C.c_void_p(out_dev_ptr),
                                      C.c_void_p(stream or None), C.byref(wide)))
        return None, wide.value
    out = np.zeros((h, w, 3), dtype=np.uint8)
    check(lib.rtw_quantise_host(device, C.c_void_p(ptr), int(fast), w, h, C.c_void_p(out.ctypes.data),
                                C.c_void_p(stream or None), C.byref(wide)))
    return out, wide.value


def format_ppm_device(ptr: int, shape, fast: bool = False, device: int = 0, stream: int = 0):
    """rtw_format_ppm_device: the reference's PPM file of the frame at device pointer
    `ptr`, formatted on the GPU; only the text is downloaded. Returns (bytes, wide):
    the bytes equal format_ppm of the downloaded frame for every input (wide != 0: a
    channel above 1 sent the call through the host writer)."""
    h, w = int(shape[0]), int(shape[1])
    wide = C.c_uint64()
    cap = 12 * w * h + 64  # enough unless a channel is wide
    buf = C.create_string_buffer(cap)
    n = check(lib.rtw_format_ppm_device(device, C.c_void_p(ptr), int(fast), w, h, C.c_void_p(stream or None),
                                        buf, cap, C.byref(wide)))
    if n > cap:
        buf = C.create_string_buffer(n)
        check(lib.rtw_format_ppm_device(device, C.c_void_p(ptr), int(fast), w, h, C.c_void_p(stream or None),
                                        buf, n, C.byref(wide)))
    return C.string_at(buf, n), wide.value


def ppm_device_stats(device: int = 0) -> dict:
    """Kernel times (HIP events) and sizes of the last format_ppm_device on `device`."""
    st = capi.PpmStats()
    check(lib.rtw_ppm_device_stats(device, C.byref(st)))
    return st.as_dict()


PNG_TILE = 2048  # filtered bytes per deflate tile (rtw_png.h kPngTile)


def png_device(dev_ptr: int, shape, fast: bool = False, rgb8: bool = False, filter: int | None = None,
               stream: int | None = None, device: int = 0) -> bytes:
    """rtw_png_device / rtw_png_rgb8_device: the PNG file (8-bit RGB) of the frame at
    device pointer `dev_ptr` (shape (rows, W[, 3]); f64, f32 with fast=True, or the
    RGB8 image itself with rgb8=True), filtered, deflated and checksummed on the GPU;
    only the file is downloaded. filter: None = per-row choice among None/Sub/Up, or
    0, 1, 2 to force one. Blocking. png_device_stats() describes the call."""
    h, w = int(shape[0]), int(shape[1])
    f = -1 if filter is None else int(filter)
    filtered = h * (1 + 3 * w)
    cap = filtered + 5 * (filtered // PNG_TILE + 1) + 100  # a tile is never larger than stored
    buf = C.create_string_buffer(cap)
    st = C.c_void_p(stream or None)
    if rgb8:
        n = check(lib.rtw_png_rgb8_device(device, C.c_void_p(dev_ptr), w, h, f, st, buf, cap))
    else:
        n = check(lib.rtw_png_device(device, C.c_void_p(dev_ptr), int(fast), w, h, f, st, buf, cap))
    return C.string_at(buf, n)


def png_device_stats(device: int = 0) -> dict:
    """Kernel times (HIP events), tiles, rows per filter and sizes of the last png_device on `device`."""
    st = capi.PngStats()
    check(lib.rtw_png_device_stats(device, C.byref(st)))
    return st.as_dict()


def xorshift_next_int(seed: int, n: int):
    out = (capi.U128 * max(1, n))()
    check(lib.rtw_xorshift_next_int(capi.U128.of(seed), n, out))
    return [out[i].value() for i in range(n)]


def xorshift_next_01(seed: int, n: int):
    out = (C.c_double * max(1, n))()
    check(lib.rtw_xorshift_next_01(capi.U128.of(seed), n, out))
    return list(out[:n])


def seed_children(seed: int, first_pixel: int, count: int):
    out = (capi.U128 * max(1, count))()
    check(lib.rtw_seed_children(capi.U128.of(seed), first_pixel, count, out))
    return [out[i].value() for i in range(count)]


def device_count() -> int:
    n = C.c_int()
    check(lib.rtw_device_count(C.byref(n)))
    return n.value


def resolve_fast(acc_ptr: int, shape, n_samples: int, out_ptr: int = 0, preview_ptr: int = 0, device: int = 0,
                 stream: int = 0):
    """rtw_resolve_fast: (h, w, 3) u64 sums to the f32 mean frame at out_ptr and/or the
    linear RGBA8 preview at preview_ptr (0: not wanted), asynchronously on `stream`."""
    h, w = shape
    check(lib.rtw_resolve_fast(device, C.c_void_p(acc_ptr), n_samples, w, h, C.c_void_p(out_ptr or None),
                               C.c_void_p(preview_ptr or None), C.c_void_p(stream or 0)))


def lattice_stride(n: int) -> int:
    """rtw_lattice_stride: the default sample-order multiplier of an n-sample lattice (no GPU needed)."""
    return lib.rtw_lattice_stride(n)


def to_q16(v: float, limit: int) -> int:
    """The one conversion of a tolerance or luminance floor given as a fraction to the C ABI's
    q16 argument: round(v * 65536), clamped to [0, limit]."""
    return min(limit, max(0, int(math.floor(v * 65536. + 0.5))))


def adaptive_select(counts_ptr: int, mom_ptr: int, shape, n: int, tol_q16: int, floor_q16: int, list_ptr: int,
                    n_list_ptr: int, device: int = 0, stream: int = 0):
    """rtw_adaptive_select: the pixels of the (rows, w) buffers that still need samples, ascending,
    to list_ptr (rows*w u32) and their number to n_list_ptr (one u32), asynchronously on `stream`."""
    h, w = shape
    check(lib.rtw_adaptive_select(device, C.c_void_p(counts_ptr), C.c_void_p(mom_ptr), w, h, n, tol_q16, floor_q16,
                                  C.c_void_p(list_ptr), C.c_void_p(n_list_ptr), C.c_void_p(stream or 0)))


def resolve_fast_counts(acc_ptr: int, counts_ptr: int, shape, out_ptr: int = 0, preview_ptr: int = 0, device: int = 0,
                        stream: int = 0):
    """rtw_resolve_fast_counts: resolve_fast with each pixel divided by its own count (0 resolves to 0)."""
    h, w = shape
    check(lib.rtw_resolve_fast_counts(device, C.c_void_p(acc_ptr), C.c_void_p(counts_ptr), w, h,
                                      C.c_void_p(out_ptr or None), C.c_void_p(preview_ptr or None),
                                      C.c_void_p(stream or 0)))


def denoise_fast(acc_ptr: int, counts_ptr: int, mom_ptr: int, guides_ptr: int, shape, levels: int = 5,
                 normal_log2: int = 5, filter_mask: int = 0xB, sigma_l: float = 4.0, out_ptr: int = 0, var_ptr: int = 0,
                 preview_ptr: int = 0, device: int = 0, stream: int = 0):
    """rtw_denoise_fast: the guided a-trous filter of the (rows, w) sums, counts, moments and
    guides into the f32 frame at out_ptr, its variance plane at var_ptr and the RGBA8 preview at
    preview_ptr (0: not wanted), asynchronously on `stream`. levels = 0 is resolve_fast_counts."""
    h, w = shape
    prm = capi.DenoiseParams(levels, normal_log2, filter_mask, sigma_l)
    check(lib.rtw_denoise_fast(device, C.c_void_p(acc_ptr or None), C.c_void_p(counts_ptr or None),
                               C.c_void_p(mom_ptr or None), C.c_void_p(guides_ptr or None), w, h, C.byref(prm),
                               C.c_void_p(out_ptr or None), C.c_void_p(var_ptr or None),
                               C.c_void_p(preview_ptr or None), C.c_void_p(stream or 0)))


class Session:
    """Device-resident rendering (rtw_session_*): the scene lives in HBM; renders
    are enqueued on a caller HIP stream into a caller device buffer."""

    def __init__(self, device: int = 0):
        self.h = C.c_void_p()
        check(lib.rtw_session_create(device, C.byref(self.h)))

    def set_scene(self, sph, n_sph, mats, n_mats):
        check(lib.rtw_session_set_scene(self.h, sph, n_sph, mats, n_mats))

    def set_scene_moving(self, sph, n_sph, center1, mats, n_mats):
        """rtw_session_set_scene_moving: center1 holds 3 doubles per sphere, its centre at time 1
        (Scene.flatten_moving, bouncing_scene). The fast-mode sample routes then render motion blur."""
        check(lib.rtw_session_set_scene_moving(self.h, sph, n_sph, center1, mats, n_mats))

    def render(self, cam: capi.Camera, samples_sqrt: int, seed: int, out_dev_ptr: int,
               stream: int | None = None, shard=None):
        sh = _shard(shard)
        check(lib.rtw_session_render(self.h, C.byref(cam), samples_sqrt, capi.U128.of(seed),
                                     C.byref(sh) if sh is not None else None,
                                     C.c_void_p(out_dev_ptr), C.c_void_p(stream or 0)))

    def render_fast(self, cam: capi.Camera, samples_sqrt: int, seed: int, out_dev_ptr: int,
                    stream: int | None = None, shard=None):
        """f32 fast mode into an n_rows x W x 3 f32 device buffer."""
        sh = _shard(shard)
        check(lib.rtw_session_render_fast(self.h, C.byref(cam), samples_sqrt, capi.U128.of(seed),
                                          C.byref(sh) if sh is not None else None,
                                          C.c_void_p(out_dev_ptr), C.c_void_p(stream or 0)))

    def accumulate_fast(self, cam: capi.Camera, samples_sqrt: int, seed: int, acc_ptr: int, k_first: int = 0,
                        k_step: int = 1, k_count: int | None = None, shard=None, stream: int = 0):
        """Adds lattice samples k_first + i*k_step (i < k_count; default: up to the lattice's
        end) of every pixel to the n_rows x W x 3 u64 fixed-point sums at acc_ptr."""
        if k_count is None:
            n = max(1, samples_sqrt * samples_sqrt)
            k_count = (n - k_first + k_step - 1) // k_step if k_step and k_first < n else 1
        sh = _shard(shard)
        check(lib.rtw_session_accumulate_fast(self.h, C.byref(cam), samples_sqrt, capi.U128.of(seed),
                                              C.byref(sh) if sh is not None else None, k_first, k_step,
                                              k_count, C.c_void_p(acc_ptr), C.c_void_p(stream or 0)))

    def accumulate_fast_list(self, cam: capi.Camera, samples_sqrt: int, seed: int, acc_ptr: int, mom_ptr: int,
                             counts_ptr: int, m: int, k_mul: int | None = None, list_ptr: int = 0, n_list_ptr: int = 0,
                             shard=None, stream: int = 0):
        """Adds the next m samples (ordinal i is lattice sample i*k_mul mod N; default k_mul:
        lattice_stride(N)) of the pixels in the device list (list_ptr 0: every pixel) to the sums,
        the luminance moments (n_rows x W x 2 u64) and the counts (n_rows x W u32)."""
        if k_mul is None:
            k_mul = lattice_stride(max(1, samples_sqrt * samples_sqrt))
        sh = _shard(shard)
        check(lib.rtw_session_accumulate_fast_list(self.h, C.byref(cam), samples_sqrt, capi.U128.of(seed),
                                                   C.byref(sh) if sh is not None else None,
                                                   C.c_void_p(list_ptr or None), C.c_void_p(n_list_ptr or None), m, k_mul,
                                                   C.c_void_p(acc_ptr or None), C.c_void_p(mom_ptr or None),
                                                   C.c_void_p(counts_ptr or None), C.c_void_p(stream or 0)))

    def render_fast_adaptive(self, cam: capi.Camera, samples_sqrt: int, seed: int, tol: float, floor: float = 0.05,
                             min_samples: int = 16, batch: int = 16):
        """rtw_session_render_fast_adaptive (blocking): every pixel sampled until the relative
        standard error of its mean luminance sum is <= tol (against mean + floor), or the
        lattice is used up. tol and floor are fractions (to_q16). Returns (frame f32 (h, w, 3),
        counts int32 (h, w), info dict), torch tensors on the current device."""
        import torch
        h, w = cam.img_height, cam.img_width
        frame = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        counts = torch.empty((h, w), dtype=torch.int32, device="cuda")
        info = capi.AdaptiveInfo()
        check(lib.rtw_session_render_fast_adaptive(self.h, C.byref(cam), samples_sqrt, capi.U128.of(seed), None,
                                                   to_q16(tol, 65535), to_q16(floor, 1 << 24), min_samples, batch,
                                                   C.c_void_p(frame.data_ptr()), C.c_void_p(counts.data_ptr()),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream or 0),
                                                   C.byref(info)))
        return frame, counts, info.as_dict()

    def guides_fast(self, cam: capi.Camera, guides_ptr: int, shard=None, stream: int = 0):
        """rtw_session_guides_fast: (normal, bits(kind << 30 | sphere)) of every pixel's centre ray,
        one float4 each, into the n_rows x W x 4 f32 buffer at guides_ptr."""
        sh = _shard(shard)
        check(lib.rtw_session_guides_fast(self.h, C.byref(cam), C.byref(sh) if sh is not None else None,
                                          C.c_void_p(guides_ptr or None), C.c_void_p(stream or 0)))

    def render_fast_denoised(self, cam: capi.Camera, samples_sqrt: int, seed: int, tol: float = 0.0,
                             floor: float = 0.05, min_samples: int = 16, batch: int = 16, levels: int = 5,
                             normal_log2: int = 5, filter_mask: int = 0xB, sigma_l: float = 4.0):
        """rtw_session_render_fast_denoised (blocking): render_fast_adaptive's rounds (tol 0: the
        uniform frame), then guides_fast and denoise_fast. Returns (frame f32 (h, w, 3), variance
        f32 (h, w), counts int32 (h, w), info dict with denoise_ms), torch tensors."""
        import torch
        h, w = cam.img_height, cam.img_width
        frame = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        var = torch.empty((h, w), dtype=torch.float32, device="cuda")
        counts = torch.empty((h, w), dtype=torch.int32, device="cuda")
        info, ms = capi.AdaptiveInfo(), C.c_double()
        prm = capi.DenoiseParams(levels, normal_log2, filter_mask, sigma_l)
        check(lib.rtw_session_render_fast_denoised(self.h, C.byref(cam), samples_sqrt, capi.U128.of(seed), None,
                                                   to_q16(tol, 65535), to_q16(floor, 1 << 24), min_samples, batch,
                                                   C.byref(prm), C.c_void_p(frame.data_ptr()),
                                                   C.c_void_p(var.data_ptr()), C.c_void_p(counts.data_ptr()),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream or 0),
                                                   C.byref(info), C.byref(ms)))
        return frame, var, counts, dict(info.as_dict(), denoise_ms=ms.value)

    def progressive_fast(self, cam: capi.Camera, samples_sqrt: int, seed: int, passes: int):
        """Renders the lattice in `passes` strided passes (pass p: k = p mod passes) and
        yields (samples_done, frame_f32, preview_rgba8), torch tensors on the current
        device, after each. The last frame is render_fast's, bit for bit."""
        import torch
        h, w = cam.img_height, cam.img_width
        n = max(1, samples_sqrt * samples_sqrt)
        acc = torch.zeros((h, w, 3), dtype=torch.int64, device="cuda")
        frame = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        preview = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        done = 0
        for p in range(min(passes, n)):
            self.accumulate_fast(cam, samples_sqrt, seed, acc.data_ptr(), p, passes, stream=st)
            done += (n - p + passes - 1) // passes
            resolve_fast(acc.data_ptr(), (h, w), done, frame.data_ptr(), preview.data_ptr(),
                         acc.device.index, st)
            yield done, frame, preview

    def stats(self) -> capi.Stats:
        st = capi.Stats()
        check(lib.rtw_session_stats(self.h, C.byref(st)))
        return st

    def diag(self, n_pixels: int):
        """RTW_DIAG=1 renders: per-pixel (segments, clock/1024 at completion)."""
        import numpy as np
        out = np.zeros(2 * n_pixels + 4, dtype=np.uint32)
        check(lib.rtw_session_diag(self.h, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size))
        return out[:2 * n_pixels].reshape(n_pixels, 2), int(out[2 * n_pixels])

    def diag_events(self, n_pixels: int):
        """RTW_DIAG=2 renders: per pixel (segments, completion, hand-out, first park,
        first drain claim) as raw 100 MHz clock words (0: never), and the launch start."""
        import numpy as np
        out = np.zeros(5 * n_pixels + 4, dtype=np.uint32)
        check(lib.rtw_session_diag(self.h, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size))
        rec = out[:2 * n_pixels].reshape(n_pixels, 2)
        ev = out[2 * n_pixels + 4:].reshape(n_pixels, 3)
        return np.concatenate([rec, ev], axis=1), int(out[2 * n_pixels])

    def close(self):
        if self.h:
            lib.rtw_session_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rccl_available():
    """(True, "") if RCCL (librccl.so.1 with ncclGather) can be loaded, else (False,
    why). Needs no GPU."""
    buf = C.create_string_buffer(256)
    ok = lib.rtw_rccl_available(buf, len(buf))
    return bool(ok), buf.value.decode()


class Group:
    """Device-resident multi-GPU renders (rtw_group_*): one session per device entry
    (None = every visible device; an index may repeat), rows dealt cyclically, the
    row tiles gathered on the root device (entry 0) by ncclGather over xGMI when the
    entries are distinct GPUs (device copies otherwise, or when RCCL cannot be loaded
    or initialised: `stats()[2]["fallback"]` and `note()` say why) and un-permuted
    there into a caller device buffer. Blocking renders. rccl_always: RCCL even for
    one entry, an RCCL failure is an error; rccl_try: RCCL even for one entry, with
    the fallback."""

    def __init__(self, devices=None, copy_gather: bool = False, rccl_always: bool = False,
                 rccl_try: bool = False):
        self.h = C.c_void_p()
        devs = list(devices or [])
        arr = (C.c_int * max(1, len(devs)))(*devs)
        flags = ((capi.GROUP_COPY_GATHER if copy_gather else 0) | (capi.GROUP_RCCL_ALWAYS if rccl_always else 0)
                 | (capi.GROUP_RCCL_TRY if rccl_try else 0))
        check(lib.rtw_group_create(arr if devs else None, len(devs), flags, C.byref(self.h)))

    def set_scene(self, sph, n_sph, mats, n_mats):
        check(lib.rtw_group_set_scene(self.h, sph, n_sph, mats, n_mats))

    def render(self, cam: capi.Camera, samples_sqrt: int, seed: int, out_dev_ptr: int, stream: int = 0):
        """The whole image into an H x W x 3 f64 buffer on the root device, ordered after
        the work queued on `stream` (a hipStream_t handle of the root device, e.g.
        torch.cuda.current_stream().cuda_stream; 0 = the null stream)."""
        check(lib.rtw_group_render_on(self.h, C.byref(cam), samples_sqrt, capi.U128.of(seed),
                                      C.c_void_p(out_dev_ptr), C.c_void_p(stream or None)))

    def render_fast(self, cam: capi.Camera, samples_sqrt: int, seed: int, out_dev_ptr: int, stream: int = 0):
        """f32 fast mode into an H x W x 3 f32 buffer on the root device (`stream` as render)."""
        check(lib.rtw_group_render_fast_on(self.h, C.byref(cam), samples_sqrt, capi.U128.of(seed),
                                           C.c_void_p(out_dev_ptr), C.c_void_p(stream or None)))

    def stats(self):
        """(total Stats, [per-entry Stats], info dict) of the last render."""
        info = capi.GroupInfo()
        check(lib.rtw_group_stats(self.h, None, None, 0, C.byref(info)))
        total = capi.Stats()
        per = (capi.Stats * max(1, info.n_entries))()
        check(lib.rtw_group_stats(self.h, C.byref(total), per, max(1, info.n_entries), C.byref(info)))
        d = info.as_dict()
        d["gather"] = capi.GATHER_NAMES.get(info.gather, info.gather)
        d["fallback"] = capi.FALLBACK_NAMES.get(info.fallback, info.fallback)
        d["note"] = self.note()
        return total, [per[i] for i in range(info.n_entries)], d

    def note(self) -> str:
        """Why the group gathers by device copies although its entries are distinct
        GPUs ("" when it does not)."""
        return (lib.rtw_group_note(self.h) or b"").decode()

    def close(self):
        if self.h:
            lib.rtw_group_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

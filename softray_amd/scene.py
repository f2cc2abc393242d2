"""Thin object wrapper over the C ABI: one `GpuScene` per reference `Renderer` (what PreCalculate()
keeps: geometry_simple, geometry_subdivided, ExtraGeometryToRaytrace)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Frame, KernelTime, Prim


class SoftrayError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("softray error %d: %s" % (code, msg))
        self.code = code


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _check(rc):
    if rc != 0:
        raise SoftrayError(rc, _lib.lib().sr_last_error().decode())


def _vp(x):
    """A device pointer (an int; 0 / None: not given) as the C ABI takes it."""
    return C.c_void_p(x) if x else None


def _stream(stream):
    """A raw hipStream_t or a torch.cuda.Stream as the C ABI takes it."""
    return _vp(getattr(stream, "cuda_stream", stream))


def _surface_points(pos, normal, color):
    """(pos float64 [n, 3], normal float64 [n, 3], color uint32 [n] or None, n) of a point call's arrays, one entry per point."""
    pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
    normal = np.ascontiguousarray(normal, dtype=np.float64).reshape(-1, 3)
    if normal.shape[0] != pos.shape[0]:
        raise ValueError("normal has %d entries for %d points" % (normal.shape[0], pos.shape[0]))
    if color is not None:
        color = np.ascontiguousarray(color, dtype=np.uint32).reshape(-1)
        if color.size != pos.shape[0]:
            raise ValueError("color has %d entries for %d points" % (color.size, pos.shape[0]))
    return pos, normal, color, pos.shape[0]


def _hit_arrays(n):
    """The six arrays a trace of n rays answers with, keyed like trace()'s result."""
    return dict(hit=np.zeros(n, dtype=np.uint8), ray_frac=np.zeros(n), pos=np.zeros((n, 3)),
                normal=np.zeros((n, 3)), color=np.zeros(n, dtype=np.uint32), tri_index=np.zeros(n, dtype=np.int32))


class GpuScene:
    def __init__(self, device=0, devices=None):
        """device: one HIP ordinal (-1 = host-only scene); devices: a list of ordinals -> ONE scene over several GPUs of this
        process (sr_create_multi: frames are split into interleaved 16-row strips inside the library)."""
        h = C.c_void_p()
        if devices is not None:
            arr = (C.c_int32 * len(devices))(*[int(d) for d in devices])
            _check(_lib.lib().sr_create_multi(arr, len(devices), C.byref(h)))
            device = int(devices[0]) if len(devices) else -1
        else:
            _check(_lib.lib().sr_create(int(device), C.byref(h)))
        self._h = h
        self.device = device

    def device_count(self):
        return int(_lib.lib().sr_device_count(self._h))

    def last_frame_parts(self):
        """How many parts of the scene rendered rows of the last frame (1: a single-device scene, or a frame the first device rendered whole)."""
        return int(_lib.lib().sr_last_frame_parts(self._h))

    def close(self):
        if getattr(self, "_h", None):
            try:
                _lib.lib().sr_destroy(self._h)
            except TypeError:                     # interpreter shutdown: the module globals are already gone
                pass
            self._h = None

    __del__ = close

    # ---- PreCalculate() ----
    def set_triangles(self, v9, argb, bmin, bmax):
        v9 = np.ascontiguousarray(v9, dtype=np.float64).reshape(-1, 9)
        argb = np.ascontiguousarray(argb, dtype=np.uint32)
        bmin = np.ascontiguousarray(bmin, dtype=np.float64)
        bmax = np.ascontiguousarray(bmax, dtype=np.float64)
        _check(_lib.lib().sr_set_triangles(self._h, _p(v9), _p(argb), v9.shape[0], _p(bmin), _p(bmax)))

    def set_triangles_device(self, v9, argb, bmin, bmax, stream=0, n=None):
        """sr_set_triangles_device: the model from DEVICE memory, copied and turned into records by kernels on `stream` (a raw
        hipStream_t or a torch.cuda.Stream); no host copy of the geometry is made.  v9: a contiguous float64 torch tensor [n, 3, 3] on
        the scene's device, or a raw device pointer with `n`; argb: an int32 / uint32 tensor [n] (or pointer), None = every triangle
        keeps its colour (same n as the current model).  bmin / bmax are host values."""
        self._from_device(_lib.lib().sr_set_triangles_device, v9, argb, bmin, bmax, stream, n)

    def refit_triangles_device(self, v9, argb, bmin, bmax, stream=0, n=None):
        """sr_refit_triangles_device: new vertices for a mesh that only moves -- arguments as set_triangles_device -- with the
        device-built own BVH REFIT instead of dropped: no build() is needed before the next MODE_BVH frame.  The tree keeps the shape
        of its build: after a large deformation frames get slower (never wrong), and the caller decides when to build() again."""
        self._from_device(_lib.lib().sr_refit_triangles_device, v9, argb, bmin, bmax, stream, n)

    def _from_device(self, call, v9, argb, bmin, bmax, stream, n):
        def device_array(x, what, dtypes, shape_ok):
            if x is None:
                return None, None
            if isinstance(x, int):
                if n is None:
                    raise ValueError("%s is a raw device pointer: n is needed" % what)
                return x, int(n)
            if not (hasattr(x, "data_ptr") and hasattr(x, "is_cuda")):
                raise ValueError("%s must be a torch tensor on the scene's device or a raw device pointer" % what)
            if not x.is_cuda or x.device.index != self.device:
                raise ValueError("%s is on %s, the scene on device %d" % (what, x.device, self.device))
            if str(x.dtype).replace("torch.", "") not in dtypes:
                raise ValueError("%s must be %s, not %s" % (what, " / ".join(dtypes), x.dtype))
            if not shape_ok(tuple(x.shape)) or not x.is_contiguous():
                raise ValueError("%s has shape %s%s" % (what, tuple(x.shape), "" if x.is_contiguous() else " and is not contiguous"))
            return x.data_ptr(), int(x.shape[0])
        pv, nv = device_array(v9, "v9", ("float64",), lambda s: len(s) == 3 and s[1:] == (3, 3))
        if nv is None:
            raise ValueError("v9 is needed")
        pa, na = device_array(argb, "argb", ("int32", "uint32"), lambda s: len(s) == 1)
        if na is not None and na != nv:
            raise ValueError("argb has %d entries for %d triangles" % (na, nv))
        bmin = np.ascontiguousarray(bmin, dtype=np.float64)
        bmax = np.ascontiguousarray(bmax, dtype=np.float64)
        if bmin.size != 3 or bmax.size != 3:
            raise ValueError("bmin and bmax are three doubles each")
        _check(call(self._h, _vp(pv), _vp(pa), nv, _p(bmin), _p(bmax), _stream(stream)))

    def load_3ds(self, data):
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        _check(_lib.lib().sr_load_3ds(self._h, _p(buf), buf.size))

    def num_triangles(self):
        return int(_lib.lib().sr_num_triangles(self._h))

    def get_triangles(self):
        n = self.num_triangles()
        v9 = np.zeros((n, 3, 3)); argb = np.zeros(n, dtype=np.uint32); bmin = np.zeros(3); bmax = np.zeros(3)
        _check(_lib.lib().sr_get_triangles(self._h, _p(v9), _p(argb), _p(bmin), _p(bmax)))
        return v9, argb, bmin, bmax

    def set_extra(self, prims):
        arr = (Prim * max(1, len(prims)))()
        for i, (kind, argb, params) in enumerate(prims):
            arr[i].kind = kind
            arr[i].argb = argb
            for j, v in enumerate(params):
                arr[i].p[j] = v
        _check(_lib.lib().sr_set_extra_geometry(self._h, arr, len(prims)))

    def build(self, modes=(_lib.MODE_REF_TREE,), max_depth=0, max_per_leaf=0, on_device=None):
        """on_device: None = the library's default for the own BVH (device LBVH when the scene has a device), True = insist on the
        device build, False = the host's binned-SAH builder."""
        mask = 0 if on_device is None else (_lib.BUILD_ON_DEVICE if on_device else _lib.BUILD_ON_HOST)
        for m in modes:
            mask |= 1 << m
        _check(_lib.lib().sr_build(self._h, mask, max_depth, max_per_leaf))

    def tree_stats(self):
        out = np.zeros(4, dtype=np.int32)
        _check(_lib.lib().sr_tree_stats(self._h, _p(out)))
        return tuple(int(x) for x in out)

    def tree_handle_leaf(self, tri):
        """(box float64 [6] = lo x 3, hi x 3 with the containment test's 1e-10 slack, members int32 [k] in the leaf's order) of the reference tree's
        leaf that listed triangle `tri` last: what the second stage of the triangle light field searches (sr_tree_handle_leaf)."""
        box = np.zeros(6)
        n = int(_lib.lib().sr_tree_handle_leaf(self._h, int(tri), _p(box), None, 0))
        _check(min(n, 0))
        members = np.zeros(n, dtype=np.int32)
        _check(min(int(_lib.lib().sr_tree_handle_leaf(self._h, int(tri), _p(box), _p(members), n)), 0))
        return box, members

    def bvh_stats(self):
        """(depth, inner nodes, triangles, built on device) of the library's own BVH."""
        out = np.zeros(4, dtype=np.int64)
        _check(_lib.lib().sr_bvh_stats(self._h, _p(out)))
        return tuple(int(x) for x in out)

    def wide_tree_stats(self):
        """(depth, nodes, child slots in use, leaves, triangles in leaves) of the four-wide form of the own BVH (host- or device-built)."""
        out = np.zeros(5, dtype=np.int64)
        _check(_lib.lib().sr_wide_tree_stats(self._h, _p(out)))
        return tuple(int(x) for x in out)

    def bvh_digest(self):
        """(hash of the node array, hash of the leaf-ordered triangle indices) of the host-built BVH."""
        out = np.zeros(2, dtype=np.uint64)
        _check(_lib.lib().sr_bvh_digest(self._h, _p(out)))
        return tuple(int(x) for x in out)

    # ---- rayTraceVoxels (SR_F_VOXELS frames, TARGET_VOXELS rays) ----
    def build_voxels(self):
        """TriMeshToVoxelGrid.Convert for the current triangles (idempotent; the first voxel frame calls it itself)."""
        _check(_lib.lib().sr_build_voxels(self._h))

    @property
    def voxel_res(self):
        """N of the N^3 voxel grid (VoxelGrid(N, ...)): 1..256, default 64 (Renderer.cs:1570).  Another value drops the grid."""
        return int(_lib.lib().sr_get_voxel_res(self._h))

    @voxel_res.setter
    def voxel_res(self, n):
        _check(_lib.lib().sr_set_voxel_res(self._h, int(n)))

    def get_voxels(self):
        """(colors uint32 [N, N, N], normals float64 [N, N, N, 3]) of the grid, [x][y][z], N = voxel_res; also for a host-only scene."""
        n = self.voxel_res
        colors = np.zeros((n, n, n), dtype=np.uint32)
        normals = np.zeros((n, n, n, 3))
        _check(_lib.lib().sr_get_voxels(self._h, _p(colors), _p(normals)))
        return colors, normals

    # ---- Render() ----
    @staticmethod
    def pixel_count(frame):
        return int(_lib.lib().sr_frame_pixel_count(C.byref(frame)))

    def render(self, frame, out=None, stats=True):
        n = self.pixel_count(frame)
        if out is not None:
            if not (isinstance(out, np.ndarray) and out.dtype.itemsize == 4 and out.dtype.kind in "iu" and out.flags["C_CONTIGUOUS"]
                    and out.flags["WRITEABLE"] and out.size >= n):
                raise ValueError("out must be a writable C-contiguous int32/uint32 array of at least %d pixels" % n)
        pixels = out if out is not None else np.zeros(n, dtype=np.int32)
        st = np.zeros(4, dtype=np.uint64) if stats else None
        _check(_lib.lib().sr_render(self._h, C.byref(frame), _p(pixels), _p(st)))
        return pixels.view(np.uint32), st

    def render_device(self, frame, d_pixels_ptr, stream=0, d_stats_ptr=None):
        _check(_lib.lib().sr_render_device(self._h, C.byref(frame), C.c_void_p(d_pixels_ptr), C.c_void_p(stream),
                                           C.c_void_p(d_stats_ptr) if d_stats_ptr else None))

    # ---- PostProcessImage / AntiAliasImage (Renderer.cs:765-767) ----
    def post_process(self, pixels, style, background_color=0):
        """In place on a host int32/uint32 array."""
        assert pixels.dtype.itemsize == 4 and pixels.flags["C_CONTIGUOUS"]
        _check(_lib.lib().sr_post_process(self._h, _p(pixels), pixels.size, int(style), int(background_color) & 0xFFFFFFFF))
        return pixels

    def post_process_device(self, d_pixels_ptr, count, style, background_color=0, stream=0):
        _check(_lib.lib().sr_post_process_device(self._h, C.c_void_p(d_pixels_ptr), int(count), int(style),
                                                 int(background_color) & 0xFFFFFFFF, C.c_void_p(stream)))

    def anti_alias(self, src, dst_width, dst_height, resolution, out=None):
        src = np.ascontiguousarray(src)
        assert src.dtype.itemsize == 4 and (resolution < 1 or src.size == dst_width * dst_height * resolution * resolution)
        dst = out if out is not None else np.zeros(dst_width * dst_height, dtype=np.int32)
        _check(_lib.lib().sr_anti_alias(self._h, _p(src), int(dst_width), int(dst_height), int(resolution), _p(dst)))
        return dst.view(np.uint32)

    def anti_alias_device(self, d_src_ptr, dst_width, dst_height, resolution, d_dst_ptr, stream=0):
        _check(_lib.lib().sr_anti_alias_device(self._h, C.c_void_p(d_src_ptr), int(dst_width), int(dst_height), int(resolution),
                                               C.c_void_p(d_dst_ptr), C.c_void_p(stream)))

    def reset_shadow_cache(self):
        """Forget the static shadow cache (SR_F_STATIC_SHADOWS): what a new Renderer starts with."""
        _check(_lib.lib().sr_reset_shadow_cache(self._h))

    def get_shadow_cache(self):
        """The static shadow cache as uint8 [128, 128, 128] in x, y, z order (0 = empty cell): the bytes of the reference's
        softShadow_..._res128.cache file."""
        out = np.zeros((_lib.AO_RES,) * 3, dtype=np.uint8)
        _check(_lib.lib().sr_get_shadow_cache(self._h, _p(out)))
        return out

    def set_shadow_cache(self, cache):
        cache = np.ascontiguousarray(cache, dtype=np.uint8)
        if cache.size != _lib.AO_RES ** 3:
            raise ValueError("the static shadow cache is %d^3 bytes" % _lib.AO_RES)
        _check(_lib.lib().sr_set_shadow_cache(self._h, _p(cache)))

    # ---- rayTraceAmbientOcclusion (SR_F_AMBIENT_OCCLUSION frames) ----
    def reset_ao_cache(self):
        """Forget the ambient-occlusion cache: what a new Renderer starts with."""
        _check(_lib.lib().sr_reset_ao_cache(self._h))

    def get_ao_cache(self):
        """The cache as uint8 [128, 128, 128] in x, y, z order (0 = empty cell): the array the reference persists to its .ao file."""
        out = np.zeros((_lib.AO_RES,) * 3, dtype=np.uint8)
        _check(_lib.lib().sr_get_ao_cache(self._h, _p(out)))
        return out

    def set_ao_cache(self, cache):
        cache = np.ascontiguousarray(cache, dtype=np.uint8)
        if cache.size != _lib.AO_RES ** 3:
            raise ValueError("the ambient-occlusion cache is %d^3 bytes" % _lib.AO_RES)
        _check(_lib.lib().sr_set_ao_cache(self._h, _p(cache)))

    # ---- rayTraceLightField (SR_F_LIGHT_FIELD frames) ----
    @property
    def light_field_res(self):
        """N of the light field's 4 N^4 entries (default 64, the reference's lightFieldRes); setting another value drops the table."""
        return int(_lib.lib().sr_get_light_field_res(self._h))

    @light_field_res.setter
    def light_field_res(self, n):
        _check(_lib.lib().sr_set_light_field_res(self._h, int(n)))

    @property
    def light_field_shadows(self):
        """Whether SR_F_LIGHT_FIELD | SR_F_SHADOWS (dynamic) is accepted: the table then stores shadowed colours (sr_set_light_field_shadows)."""
        return bool(_lib.lib().sr_get_light_field_shadows(self._h))

    @light_field_shadows.setter
    def light_field_shadows(self, on):
        _check(_lib.lib().sr_set_light_field_shadows(self._h, 1 if on else 0))

    @property
    def light_field_interpolation(self):
        """Whether SR_F_LIGHT_FIELD frames blend the 16 entries around a sample's 4-D coordinate (sr_set_light_field_interpolation)."""
        return bool(_lib.lib().sr_get_light_field_interpolation(self._h))

    @light_field_interpolation.setter
    def light_field_interpolation(self, on):
        _check(_lib.lib().sr_set_light_field_interpolation(self._h, 1 if on else 0))

    @property
    def light_field_triangles(self):
        """Whether SR_F_LIGHT_FIELD frames and bake_light_field run the triangle-index light field (LightFieldStoresTriangles = true) on the triangle
        table instead of the colour light field on the colour table (sr_set_light_field_triangles)."""
        return bool(_lib.lib().sr_get_light_field_triangles(self._h))

    @light_field_triangles.setter
    def light_field_triangles(self, on):
        _check(_lib.lib().sr_set_light_field_triangles(self._h, 1 if on else 0))

    def get_light_field_tris(self, first=0, count=None):
        """Entries first .. first + count - 1 (default: all 4 N^4) of the triangle table as uint32: 0 empty, 1 nothing, t + 2 triangle t."""
        total = 4 * self.light_field_res ** 4
        if count is None:
            count = total - first
        out = np.zeros(int(count), dtype=np.uint32)
        _check(_lib.lib().sr_get_light_field_tris(self._h, _p(out), int(first), int(count)))
        return out

    def set_light_field_tris(self, entries, first=0):
        entries = np.ascontiguousarray(entries, dtype=np.uint32).reshape(-1)
        _check(_lib.lib().sr_set_light_field_tris(self._h, _p(entries), int(first), int(entries.size)))

    def light_field_coords(self, starts, dirs):
        """LightField4D.RayToFloat4D of every line (sr_light_field_coords), computed on the device at light_field_res: (float64 [n, 4], bool [n] --
        False: the line misses the sphere and its coordinates are 0)."""
        starts = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        if dirs.shape[0] != starts.shape[0]:
            raise ValueError("starts and dirs must have the same length")
        coords = np.zeros((starts.shape[0], 4), dtype=np.float64)
        inside = np.zeros(starts.shape[0], dtype=np.uint8)
        _check(_lib.lib().sr_light_field_coords(self._h, starts.shape[0], _p(starts), _p(dirs), _p(coords), _p(inside)))
        return coords, inside.astype(bool)

    def reset_light_field(self):
        """Forget the light field: what a new Renderer starts with."""
        _check(_lib.lib().sr_reset_light_field(self._h))

    def get_light_field(self, first=0, count=None):
        """Entries first .. first + count - 1 (default: all 4 N^4) as uint32, 0 = empty: the array the reference persists to its .cache file."""
        total = 4 * self.light_field_res ** 4
        if count is None:
            count = total - first
        out = np.zeros(int(count), dtype=np.uint32)
        _check(_lib.lib().sr_get_light_field(self._h, _p(out), int(first), int(count)))
        return out

    def set_light_field(self, entries, first=0):
        entries = np.ascontiguousarray(entries, dtype=np.uint32).reshape(-1)
        _check(_lib.lib().sr_set_light_field(self._h, _p(entries), int(first), int(entries.size)))

    def bake_light_field(self, frame, first=0, count=None):
        """Fill every empty entry of first .. first + count - 1 (default: to the end of the table) with the colour of its cell's canonical ray, as a
        light-field frame with `frame`'s geometry, shading and lights would; returns the number of entries written (sr_bake_light_field)."""
        if count is None:
            count = 4 * self.light_field_res ** 4 - int(first)
        filled = C.c_uint64(0)
        _check(_lib.lib().sr_bake_light_field(self._h, C.byref(frame), int(first), int(count), C.byref(filled)))
        return int(filled.value)

    def ray_stats(self):
        """primary {rays, tests, nodes, leaves} + secondary {rays, tests, nodes, leaves} of the last render(stats=True)."""
        out = np.zeros(24, dtype=np.uint64)                           # SR_STATS_COUNT
        _check(_lib.lib().sr_last_ray_stats(self._h, _p(out)))
        return out

    def debug_set(self, key, value):
        """Test / experiment hook of this scene (include/softray.h SR_DBG_*); value < 0 restores the default."""
        _check(_lib.lib().sr_debug_set(self._h, int(key), int(value)))

    def debug_counters(self):
        out = np.zeros(8, dtype=np.uint32)
        _check(_lib.lib().sr_debug_counters(self._h, _p(out)))
        return [int(x) for x in out]

    def reset_kernel_times(self):
        _lib.lib().sr_reset_kernel_times(self._h)

    def kernel_times(self):
        """{kernel: (total ms, launches)} since reset_kernel_times() -- HIP events on the launch stream."""
        arr = (KernelTime * 64)()
        n = _lib.lib().sr_kernel_times(self._h, arr, 64)
        return {arr[i].name.decode(): (float(arr[i].ms), int(arr[i].launches)) for i in range(n)}

    def shade_points(self, frame, pos, normal, color):
        """ShadingMethod.IntersectRay's colour step for recorded intersections (sr_shade_points)."""
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        normal = np.ascontiguousarray(normal, dtype=np.float64).reshape(-1, 3)
        color = np.ascontiguousarray(color, dtype=np.uint32)
        out = np.zeros(pos.shape[0], dtype=np.uint32)
        _check(_lib.lib().sr_shade_points(self._h, C.byref(frame), pos.shape[0], _p(pos), _p(normal), _p(color), _p(out)))
        return out

    def shadow_points(self, frame, pos, normal, color=None, coherent=False):
        """ShadowMethod's soft shadow for caller-given surface points (sr_shadow_points): uint32 [n], color[i] (None: 0xFFFFFFFF) modulated
        with the byte of the frame's light, samples and root geometry.  coherent: 64 consecutive points are neighbours (no ray sort)."""
        pos, normal, color, n = _surface_points(pos, normal, color)
        out = np.zeros(n, dtype=np.uint32)
        _check(_lib.lib().sr_shadow_points(self._h, C.byref(frame), n, _p(pos), _p(normal), _p(color), _p(out),
                                           _lib.POINTS_COHERENT if coherent else 0))
        return out

    def shadow_points_device(self, frame, n, d_pos, d_normal, d_color, d_out, coherent=False, stream=0, d_stats_ptr=None):
        """sr_shadow_points_device: every array is a DEVICE pointer (d_color 0 / None: every point 0xFFFFFFFF; d_out may be d_color);
        enqueued on `stream` (a raw hipStream_t or a torch.cuda.Stream), no host sync."""
        _check(_lib.lib().sr_shadow_points_device(self._h, C.byref(frame), int(n), _vp(d_pos), _vp(d_normal), _vp(d_color), _vp(d_out),
                                                  _lib.POINTS_COHERENT if coherent else 0, _stream(stream), _vp(d_stats_ptr)))

    def static_shadow_points(self, frame, pos, normal, color=None, coherent=False, want_out=True, want_amount=True):
        """ShadowMethod's static branch for caller-given surface points, in input order (sr_static_shadow_points): (out uint32 [n] or None,
        amount uint8 [n] or None, generators).  The first point of an empty cell of the scene's static shadow cache generates the cell's
        byte; every point reads its cell.  color None: every point 0xFFFFFFFF.  coherent: the generators of a pass are neighbours in input
        order (no sort)."""
        pos, normal, color, n = _surface_points(pos, normal, color)
        out = np.zeros(n, dtype=np.uint32) if want_out else None
        amount = np.zeros(n, dtype=np.uint8) if want_amount else None
        made = C.c_uint64(0)
        _check(_lib.lib().sr_static_shadow_points(self._h, C.byref(frame), n, _p(pos), _p(normal), _p(color), _p(out), _p(amount),
                                                  _lib.POINTS_COHERENT if coherent else 0, C.byref(made)))
        return out, amount, int(made.value)

    def static_shadow_points_device(self, frame, n, d_pos, d_normal, d_color, d_out, d_amount, coherent=False, stream=0, d_generators_ptr=None,
                                    d_stats_ptr=None):
        """sr_static_shadow_points_device: every array is a DEVICE pointer (d_color 0 / None: every point 0xFFFFFFFF; d_out may be d_color; one
        of d_out / d_amount may be 0 / None; d_generators_ptr: a device uint64 or None); enqueued on `stream` (a raw hipStream_t or a
        torch.cuda.Stream), no host sync."""
        _check(_lib.lib().sr_static_shadow_points_device(self._h, C.byref(frame), int(n), _vp(d_pos), _vp(d_normal), _vp(d_color), _vp(d_out),
                                                         _vp(d_amount), _lib.POINTS_COHERENT if coherent else 0, _stream(stream), _vp(d_generators_ptr),
                                                         _vp(d_stats_ptr)))

    def ao_points(self, frame, pos, normal, color=None, first_generator=0, want_out=True, want_amount=True):
        """AmbientOcclusionMethod's step for caller-given surface points, in input order (sr_ao_points): (out uint32 [n] or None, amount
        uint8 [n] or None, generators).  Cached in the scene's AO cache unless the frame has F_AO_UNCACHED; generator g of the call uses
        draws 300 (first_generator + g) .. + 299 of Random(frame.random_seed).  color None: every point 0xFFFFFFFF."""
        pos, normal, color, n = _surface_points(pos, normal, color)
        out = np.zeros(n, dtype=np.uint32) if want_out else None
        amount = np.zeros(n, dtype=np.uint8) if want_amount else None
        made = C.c_uint64(0)
        _check(_lib.lib().sr_ao_points(self._h, C.byref(frame), n, _p(pos), _p(normal), _p(color), _p(out), _p(amount),
                                       int(first_generator), 0, C.byref(made)))
        return out, amount, int(made.value)

    def ao_points_device(self, frame, n, d_pos, d_normal, d_color, d_out, d_amount, first_generator=0, stream=0, d_generators_ptr=None,
                         d_stats_ptr=None):
        """sr_ao_points_device: every array is a DEVICE pointer (d_color 0 / None: every point 0xFFFFFFFF; d_out may be d_color; one of d_out /
        d_amount may be 0 / None; d_generators_ptr: a device uint64 or None); enqueued on `stream` (a raw hipStream_t or a
        torch.cuda.Stream), no host sync."""
        _check(_lib.lib().sr_ao_points_device(self._h, C.byref(frame), int(n), _vp(d_pos), _vp(d_normal), _vp(d_color), _vp(d_out), _vp(d_amount),
                                              int(first_generator), 0, _stream(stream), _vp(d_generators_ptr), _vp(d_stats_ptr)))

    def path_points(self, frame, pos, normal, color=None, first_sample=0, want_out=True, want_incoming=True, want_dirs=True):
        """PathTracingMethod's step for caller-given surface points, in input order (sr_path_points): (out uint32 [n], incoming uint32 [n],
        dirs float64 [n, 3]), each None when not wanted.  Point i uses draws 3 (first_sample + i) .. + 2 of Random(frame.random_seed); a
        split batch passes first_sample + n to the next call.  color None: every point 0xFFFFFFFF."""
        pos, normal, color, n = _surface_points(pos, normal, color)
        out = np.zeros(n, dtype=np.uint32) if want_out else None
        incoming = np.zeros(n, dtype=np.uint32) if want_incoming else None
        dirs = np.zeros((n, 3), dtype=np.float64) if want_dirs else None
        _check(_lib.lib().sr_path_points(self._h, C.byref(frame), n, _p(pos), _p(normal), _p(color), _p(out), _p(incoming), _p(dirs),
                                         int(first_sample), 0))
        return out, incoming, dirs

    def path_points_device(self, frame, n, d_pos, d_normal, d_color, d_out, d_incoming=None, d_dirs=None, first_sample=0, stream=0, d_stats_ptr=None):
        """sr_path_points_device: every array is a DEVICE pointer (d_color 0 / None: every point 0xFFFFFFFF; d_out may be d_color; d_out,
        d_incoming and d_dirs may each be 0 / None, not all three); enqueued on `stream` (a raw hipStream_t or a torch.cuda.Stream), no
        host sync."""
        _check(_lib.lib().sr_path_points_device(self._h, C.byref(frame), int(n), _vp(d_pos), _vp(d_normal), _vp(d_color), _vp(d_out), _vp(d_incoming),
                                                _vp(d_dirs), int(first_sample), 0, _stream(stream), _vp(d_stats_ptr)))

    def shade_points_device(self, frame, n, d_pos, d_normal, d_color, d_out, stream=0):
        """sr_shade_points_device: every array is a DEVICE pointer; enqueued on `stream` (a raw hipStream_t or a torch.cuda.Stream), no host sync."""
        _check(_lib.lib().sr_shade_points_device(self._h, C.byref(frame), int(n), _vp(d_pos), _vp(d_normal), _vp(d_color), _vp(d_out), _stream(stream)))

    # ---- the frame G-buffer: the primary stage's answer per camera sample (sr_render_hits) ----
    @staticmethod
    def sample_count(frame):
        """Camera samples of the frame: rows x width x sub_pixel_res^2 of the clamped row range (sr_frame_sample_count)."""
        return int(_lib.lib().sr_frame_sample_count(C.byref(frame)))

    def render_hits(self, frame, rays=False, stats=False):
        """Per camera sample of `frame`, in scan order ((row - first row) * width + col) * n^2 + subX * n + subY: a dict keyed like trace()'s
        result (hit, ray_frac, pos, normal, color, tri_index), with rays=True also the camera rays (starts, dirs), with stats=True the four
        primary counters (stats)."""
        n = self.sample_count(frame)
        res = _hit_arrays(n)
        if rays:
            res["starts"], res["dirs"] = np.zeros((n, 3)), np.zeros((n, 3))
        st = np.zeros(4, dtype=np.uint64) if stats else None
        _check(_lib.lib().sr_render_hits(self._h, C.byref(frame), _p(res.get("starts")), _p(res.get("dirs")), _p(res["hit"]), _p(res["ray_frac"]),
                                         _p(res["pos"]), _p(res["normal"]), _p(res["color"]), _p(res["tri_index"]), _p(st)))
        if stats:
            res["stats"] = st
        return res

    def render_hits_device(self, frame, d_starts=0, d_dirs=0, d_hit=0, d_ray_frac=0, d_pos=0, d_normal=0, d_color=0, d_tri_index=0, stream=0,
                           d_stats_ptr=None):
        """sr_render_hits_device: every array is a DEVICE pointer (0 / None: not wanted) with room for sample_count(frame) entries; enqueued on
        `stream` (a raw hipStream_t or a torch.cuda.Stream), no host sync."""
        _check(_lib.lib().sr_render_hits_device(self._h, C.byref(frame), _vp(d_starts), _vp(d_dirs), _vp(d_hit), _vp(d_ray_frac), _vp(d_pos), _vp(d_normal),
                                                _vp(d_color), _vp(d_tri_index), _stream(stream), _vp(d_stats_ptr)))

    # ---- IRayIntersectable.IntersectRay, batched ----
    def trace(self, target, starts, dirs, counters=False):
        starts = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        n = starts.shape[0]
        res = _hit_arrays(n)
        cnt = np.zeros((n, 3), dtype=np.int32) if counters else None
        _check(_lib.lib().sr_trace_rays(self._h, int(target), n, _p(starts), _p(dirs), _p(res["hit"]), _p(res["ray_frac"]),
                                        _p(res["pos"]), _p(res["normal"]), _p(res["color"]), _p(res["tri_index"]), _p(cnt)))
        if counters:
            res["counters"] = cnt
        return res


    def trace_device(self, target, n, d_starts, d_dirs, d_hit=0, d_ray_frac=0, d_pos=0, d_normal=0, d_color=0, d_tri_index=0, d_counters=0, stream=0):
        """sr_trace_rays_device: every array is a DEVICE pointer (e.g. tensor.data_ptr()); enqueued on `stream`, no host sync."""
        _check(_lib.lib().sr_trace_rays_device(self._h, int(target), int(n), _vp(d_starts), _vp(d_dirs), _vp(d_hit), _vp(d_ray_frac), _vp(d_pos),
                                               _vp(d_normal), _vp(d_color), _vp(d_tri_index), _vp(d_counters), _vp(stream)))

    # ---- a ray batch from one origin on the frame's packet walk (sr_trace_origin_rays) ----
    def trace_origin(self, target, origin, dirs, coherent=False, stats=False):
        """trace(target, tile(origin), dirs), bit for bit, on the walk a frame's camera rays take: a dict with trace()'s keys (with
        stats=True also the four primary counters, `stats`).  coherent: every 64 consecutive rays are neighbours (SR_RAYS_COHERENT)."""
        origin = np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
        dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        n = dirs.shape[0]
        res = _hit_arrays(n)
        st = np.zeros(4, dtype=np.uint64) if stats else None
        _check(_lib.lib().sr_trace_origin_rays(self._h, int(target), _p(origin), n, _p(dirs), _p(res["hit"]), _p(res["ray_frac"]), _p(res["pos"]),
                                               _p(res["normal"]), _p(res["color"]), _p(res["tri_index"]), _lib.RAYS_COHERENT if coherent else 0, _p(st)))
        if stats:
            res["stats"] = st
        return res

    def trace_origin_device(self, target, origin, n, d_dirs, d_hit=0, d_ray_frac=0, d_pos=0, d_normal=0, d_color=0, d_tri_index=0, coherent=False,
                            stream=0, d_stats_ptr=None):
        """sr_trace_origin_rays_device: `origin` is a host triple, every array a DEVICE pointer (0 / None: not wanted); enqueued on `stream` (a raw
        hipStream_t or a torch.cuda.Stream), no host sync."""
        origin = np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
        _check(_lib.lib().sr_trace_origin_rays_device(self._h, int(target), _p(origin), int(n), _vp(d_dirs), _vp(d_hit), _vp(d_ray_frac), _vp(d_pos),
                                                      _vp(d_normal), _vp(d_color), _vp(d_tri_index), _lib.RAYS_COHERENT if coherent else 0, _stream(stream),
                                                      _vp(d_stats_ptr)))

    # ---- any-hit ray batches with a distance limit (sr_occluded_rays) ----
    @staticmethod
    def _ray_options(endpoints, coherent):
        return (_lib.RAYS_ENDPOINTS if endpoints else 0) | (_lib.RAYS_COHERENT if coherent else 0)

    def occluded(self, target, starts, dirs, limits=None, endpoints=False, coherent=False, stats=False):
        """uint8 [n]: trace(target, starts, D) answers hit and ray_frac <= limit (limits None: 1.0 for every ray), with early exit on the own
        BVH.  D = dirs, or dirs - starts with endpoints=True (dirs are end points).  stats=True: (occluded, the four counters)."""
        starts = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        n = starts.shape[0]
        if dirs.shape[0] != n:
            raise ValueError("dirs has %d entries for %d rays" % (dirs.shape[0], n))
        if limits is not None:
            limits = np.ascontiguousarray(limits, dtype=np.float64).reshape(-1)
            if limits.size != n:
                raise ValueError("limits has %d entries for %d rays" % (limits.size, n))
        out = np.zeros(n, dtype=np.uint8)
        st = np.zeros(4, dtype=np.uint64) if stats else None
        _check(_lib.lib().sr_occluded_rays(self._h, int(target), n, _p(starts), _p(dirs), _p(limits), _p(out), self._ray_options(endpoints, coherent), _p(st)))
        return (out, st) if stats else out

    def occluded_device(self, target, n, d_starts, d_dirs, d_limits=0, d_occluded=0, endpoints=False, coherent=False, stream=0, d_stats_ptr=None):
        """sr_occluded_rays_device: every array is a DEVICE pointer (d_limits 0 / None: 1.0 for every ray); enqueued on `stream` (a raw
        hipStream_t or a torch.cuda.Stream), no host sync."""
        _check(_lib.lib().sr_occluded_rays_device(self._h, int(target), int(n), _vp(d_starts), _vp(d_dirs), _vp(d_limits), _vp(d_occluded),
                                                  self._ray_options(endpoints, coherent), _stream(stream), _vp(d_stats_ptr)))

    # ---- nearest-hit ray batches with a distance limit (sr_nearest_rays) ----
    def nearest(self, target, starts, dirs, limits=None, endpoints=False, coherent=False, stats=False):
        """trace(target, starts, D) where that is a hit with ray_frac <= limit, trace()'s miss otherwise (limits None: no limit), on the walk the
        library keeps for incoherent rays: a dict with trace()'s keys (with stats=True also the four counters, `stats`).  D = dirs, or
        dirs - starts with endpoints=True (dirs are end points)."""
        starts = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        n = starts.shape[0]
        if dirs.shape[0] != n:
            raise ValueError("dirs has %d entries for %d rays" % (dirs.shape[0], n))
        if limits is not None:
            limits = np.ascontiguousarray(limits, dtype=np.float64).reshape(-1)
            if limits.size != n:
                raise ValueError("limits has %d entries for %d rays" % (limits.size, n))
        res = _hit_arrays(n)
        st = np.zeros(4, dtype=np.uint64) if stats else None
        _check(_lib.lib().sr_nearest_rays(self._h, int(target), n, _p(starts), _p(dirs), _p(limits), _p(res["hit"]), _p(res["ray_frac"]), _p(res["pos"]),
                                          _p(res["normal"]), _p(res["color"]), _p(res["tri_index"]), self._ray_options(endpoints, coherent), _p(st)))
        if stats:
            res["stats"] = st
        return res

    def nearest_device(self, target, n, d_starts, d_dirs, d_limits=0, d_hit=0, d_ray_frac=0, d_pos=0, d_normal=0, d_color=0, d_tri_index=0, endpoints=False,
                       coherent=False, stream=0, d_stats_ptr=None):
        """sr_nearest_rays_device: every array is a DEVICE pointer (d_limits 0 / None: no limit; an output 0 / None: not wanted); enqueued on
        `stream` (a raw hipStream_t or a torch.cuda.Stream), no host sync."""
        _check(_lib.lib().sr_nearest_rays_device(self._h, int(target), int(n), _vp(d_starts), _vp(d_dirs), _vp(d_limits), _vp(d_hit), _vp(d_ray_frac),
                                                 _vp(d_pos), _vp(d_normal), _vp(d_color), _vp(d_tri_index), self._ray_options(endpoints, coherent),
                                                 _stream(stream), _vp(d_stats_ptr)))

    # ---- all hits along a ray, nearest first, with a count (sr_all_hits_rays) ----
    def all_hits(self, target, starts, dirs, limits=None, max_hits=8, want_count=True, endpoints=False, coherent=False, stats=False):
        """Every hit of every ray with ray_frac <= limit (limits None: no limit): a dict with `count` (uint32 [n], not capped by max_hits; None
        with want_count=False, which lets the walk cull beyond the max_hits-th hit), `index` (int32 [n][max_hits]: TriangleIndex, -2 - e for extra
        element e, -1 in unused slots) and `ray_frac` (float64 [n][max_hits], 0.0 in unused slots), rows ordered by (ray_frac, extra elements
        first, index); with stats=True also the four counters, `stats`.  max_hits=0 is the counting call.  D = dirs, or dirs - starts with
        endpoints=True."""
        starts = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        n = starts.shape[0]
        if dirs.shape[0] != n:
            raise ValueError("dirs has %d entries for %d rays" % (dirs.shape[0], n))
        if limits is not None:
            limits = np.ascontiguousarray(limits, dtype=np.float64).reshape(-1)
            if limits.size != n:
                raise ValueError("limits has %d entries for %d rays" % (limits.size, n))
        k = int(max_hits)
        rows = max(0, min(k, _lib.HITS_MAX))
        res = {"count": np.zeros(n, dtype=np.uint32) if want_count else None,
               "index": np.full((n, rows), -1, dtype=np.int32), "ray_frac": np.zeros((n, rows), dtype=np.float64)}
        st = np.zeros(4, dtype=np.uint64) if stats else None
        _check(_lib.lib().sr_all_hits_rays(self._h, int(target), n, _p(starts), _p(dirs), _p(limits), k, _p(res["count"]),
                                           _p(res["index"]) if rows else None, _p(res["ray_frac"]) if rows else None,
                                           self._ray_options(endpoints, coherent), _p(st)))
        if stats:
            res["stats"] = st
        return res

    def all_hits_device(self, target, n, d_starts, d_dirs, d_limits=0, max_hits=8, d_count=0, d_index=0, d_ray_frac=0, endpoints=False, coherent=False,
                        stream=0, d_stats_ptr=None):
        """sr_all_hits_rays_device: every array is a DEVICE pointer (d_limits 0 / None: no limit; an output 0 / None: not wanted); enqueued on
        `stream` (a raw hipStream_t or a torch.cuda.Stream), no host sync."""
        _check(_lib.lib().sr_all_hits_rays_device(self._h, int(target), int(n), _vp(d_starts), _vp(d_dirs), _vp(d_limits), int(max_hits), _vp(d_count),
                                                  _vp(d_index), _vp(d_ray_frac), self._ray_options(endpoints, coherent), _stream(stream), _vp(d_stats_ptr)))

    # ---- the closest point of the mesh for a batch of points (sr_closest_points) ----
    def closest_points(self, target, points, max_dist=None, want=("tri_index", "dist", "pos", "uv"), coherent=False, stats=False):
        """For every point the triangle that minimises (squared distance, TriangleIndex), where its distance is <= max_dist (None: no limit):
        a dict with `tri_index` (int32 [n], -1: no qualifying answer), `dist` (float64 [n]), `pos` (float64 [n][3], the closest point) and `uv`
        (float64 [n][2], the weights of vertices 2 and 3); zeros where tri_index is -1.  `want` names the outputs asked for (the others are
        None); with stats=True also the four counters, `stats`.  target: MODE_BVH or MODE_BRUTE."""
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n = points.shape[0]
        if max_dist is not None:
            max_dist = np.ascontiguousarray(max_dist, dtype=np.float64).reshape(-1)
            if max_dist.size != n:
                raise ValueError("max_dist has %d entries for %d points" % (max_dist.size, n))
        res = {"tri_index": np.full(n, -1, dtype=np.int32) if "tri_index" in want else None,
               "dist": np.zeros(n, dtype=np.float64) if "dist" in want else None,
               "pos": np.zeros((n, 3), dtype=np.float64) if "pos" in want else None,
               "uv": np.zeros((n, 2), dtype=np.float64) if "uv" in want else None}
        st = np.zeros(4, dtype=np.uint64) if stats else None
        _check(_lib.lib().sr_closest_points(self._h, int(target), n, _p(points), _p(max_dist), _p(res["tri_index"]), _p(res["dist"]), _p(res["pos"]),
                                            _p(res["uv"]), _lib.POINTS_COHERENT if coherent else 0, _p(st)))
        if stats:
            res["stats"] = st
        return res

    def closest_points_device(self, target, n, d_points, d_max_dist=0, d_tri_index=0, d_dist=0, d_pos=0, d_uv=0, coherent=False, stream=0, d_stats_ptr=None):
        """sr_closest_points_device: every array is a DEVICE pointer (d_max_dist 0 / None: no limit; an output 0 / None: not wanted); enqueued on
        `stream` (a raw hipStream_t or a torch.cuda.Stream), no host sync."""
        _check(_lib.lib().sr_closest_points_device(self._h, int(target), int(n), _vp(d_points), _vp(d_max_dist), _vp(d_tri_index), _vp(d_dist), _vp(d_pos),
                                                   _vp(d_uv), _lib.POINTS_COHERENT if coherent else 0, _stream(stream), _vp(d_stats_ptr)))

    # ---- the triangles within reach of a point, nearest first, with a count (sr_near_triangles) ----
    def near_triangles(self, target, points, max_dist=None, max_hits=8, want=("count", "index", "dist", "pos", "uv"), coherent=False, stats=False):
        """For every point the triangles whose distance is a number <= max_dist (None: no limit): a dict with `count` (uint32 [n], not capped
        by max_hits), and rows ordered by (squared distance, TriangleIndex): `index` (int32 [n][max_hits], -1 in unused slots), `dist` (float64
        [n][max_hits]), `pos` (float64 [n][max_hits][3], the closest points) and `uv` (float64 [n][max_hits][2], the weights of vertices 2 and
        3), zeros in unused slots.  Slot 0 is closest_points' answer.  `want` names the outputs asked for (the others are None; without
        "count" the walk also culls beyond the max_hits-th entry: a K-nearest query); with stats=True also the four counters, `stats`.
        max_hits=0 is the counting call.  target: MODE_BVH or MODE_BRUTE."""
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n = points.shape[0]
        if max_dist is not None:
            max_dist = np.ascontiguousarray(max_dist, dtype=np.float64).reshape(-1)
            if max_dist.size != n:
                raise ValueError("max_dist has %d entries for %d points" % (max_dist.size, n))
        k = int(max_hits)
        rows = max(0, min(k, _lib.HITS_MAX))
        res = {"count": np.zeros(n, dtype=np.uint32) if "count" in want else None,
               "index": np.full((n, rows), -1, dtype=np.int32) if "index" in want else None,
               "dist": np.zeros((n, rows), dtype=np.float64) if "dist" in want else None,
               "pos": np.zeros((n, rows, 3), dtype=np.float64) if "pos" in want else None,
               "uv": np.zeros((n, rows, 2), dtype=np.float64) if "uv" in want else None}
        row = lambda name: _p(res[name]) if rows else None                                   # noqa: E731
        st = np.zeros(4, dtype=np.uint64) if stats else None
        _check(_lib.lib().sr_near_triangles(self._h, int(target), n, _p(points), _p(max_dist), k, _p(res["count"]), row("index"), row("dist"), row("pos"),
                                            row("uv"), _lib.POINTS_COHERENT if coherent else 0, _p(st)))
        if stats:
            res["stats"] = st
        return res

    def near_triangles_device(self, target, n, d_points, d_max_dist=0, max_hits=8, d_count=0, d_index=0, d_dist=0, d_pos=0, d_uv=0, coherent=False, stream=0,
                              d_stats_ptr=None):
        """sr_near_triangles_device: every array is a DEVICE pointer (d_max_dist 0 / None: no limit; an output 0 / None: not wanted); enqueued on
        `stream` (a raw hipStream_t or a torch.cuda.Stream), no host sync."""
        _check(_lib.lib().sr_near_triangles_device(self._h, int(target), int(n), _vp(d_points), _vp(d_max_dist), int(max_hits), _vp(d_count), _vp(d_index),
                                                   _vp(d_dist), _vp(d_pos), _vp(d_uv), _lib.POINTS_COHERENT if coherent else 0, _stream(stream), _vp(d_stats_ptr)))

    # ---- the triangles of the model that cross a triangle of the caller's (sr_overlap_triangles) ----
    def overlap_triangles(self, target, tris, max_hits=8, want=("count", "index", "mask"), coherent=False, any_hit=False, stats=False):
        """For every triangle of `tris` ([n][3][3]) the triangles of the model that cross it (the pair predicate of include/softray.h): a dict
        with `count` (uint32 [n], not capped by max_hits) and rows by ascending TriangleIndex: `index` (int32 [n][max_hits], -1 in unused
        slots) and `mask` (uint8 [n][max_hits]: bit e, the query's edge e meets the scene triangle; bit 3 + e, the scene triangle's edge e
        meets the query; 0 in unused slots).  `want` names the outputs asked for (the others are None); with stats=True also the four
        counters, `stats`.  max_hits=0 is the counting call; any_hit=True (SR_OVERLAP_ANY, max_hits must be 0): count is 0 or 1 and a query
        stops at its first triangle.  target: MODE_BVH or MODE_BRUTE."""
        tris = np.ascontiguousarray(tris, dtype=np.float64).reshape(-1, 3, 3)
        n = tris.shape[0]
        k = int(max_hits)
        rows = max(0, min(k, _lib.HITS_MAX))
        res = {"count": np.zeros(n, dtype=np.uint32) if "count" in want else None,
               "index": np.full((n, rows), -1, dtype=np.int32) if "index" in want else None,
               "mask": np.zeros((n, rows), dtype=np.uint8) if "mask" in want else None}
        row = lambda name: _p(res[name]) if rows else None                                   # noqa: E731
        st = np.zeros(4, dtype=np.uint64) if stats else None
        options = (_lib.POINTS_COHERENT if coherent else 0) | (_lib.OVERLAP_ANY if any_hit else 0)
        _check(_lib.lib().sr_overlap_triangles(self._h, int(target), n, _p(tris), k, _p(res["count"]), row("index"), row("mask"), options, _p(st)))
        if stats:
            res["stats"] = st
        return res

    def overlap_triangles_device(self, target, n, d_tris, max_hits=8, d_count=0, d_index=0, d_mask=0, coherent=False, any_hit=False, stream=0, d_stats_ptr=None):
        """sr_overlap_triangles_device: every array is a DEVICE pointer (an output 0 / None: not wanted); enqueued on `stream` (a raw
        hipStream_t or a torch.cuda.Stream), no host sync."""
        options = (_lib.POINTS_COHERENT if coherent else 0) | (_lib.OVERLAP_ANY if any_hit else 0)
        _check(_lib.lib().sr_overlap_triangles_device(self._h, int(target), int(n), _vp(d_tris), int(max_hits), _vp(d_count), _vp(d_index), _vp(d_mask), options,
                                                      _stream(stream), _vp(d_stats_ptr)))

    # ---- the colour light field for caller-given rays (sr_light_field_rays) ----
    def light_field_rays(self, frame, starts, dirs, want_inside=True):
        """LightFieldColorMethod.IntersectRay for n lines of the caller's (sr_light_field_rays): (out uint32 [n], inside uint8 [n] or None,
        filled).  out[i] is the colour a light-field frame gives a sample whose ray is (starts[i], dirs[i]) -- model space, the direction not
        normalised; empty entries of the scene's table are filled first, as a frame fills them, and `filled` counts them."""
        starts = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        n = starts.shape[0]
        if dirs.shape[0] != n:
            raise ValueError("dirs has %d entries for %d rays" % (dirs.shape[0], n))
        out = np.zeros(n, dtype=np.uint32)
        inside = np.zeros(n, dtype=np.uint8) if want_inside else None
        filled = C.c_uint64(0)
        _check(_lib.lib().sr_light_field_rays(self._h, C.byref(frame), n, _p(starts), _p(dirs), _p(out), _p(inside), 0, C.byref(filled)))
        return out, inside, int(filled.value)

    def light_field_rays_device(self, frame, n, d_starts, d_dirs, d_out, d_inside=0, stream=0, d_filled_ptr=None, d_stats_ptr=None):
        """sr_light_field_rays_device: every array is a DEVICE pointer (d_inside 0 / None: not wanted; d_filled_ptr: a device uint64 or None);
        enqueued on `stream` (a raw hipStream_t or a torch.cuda.Stream), no host sync."""
        _check(_lib.lib().sr_light_field_rays_device(self._h, C.byref(frame), int(n), _vp(d_starts), _vp(d_dirs), _vp(d_out), _vp(d_inside), 0,
                                                     _stream(stream), _vp(d_filled_ptr), _vp(d_stats_ptr)))

    # ---- the strip gather over RCCL (include/softray.h) ----
    def set_gather(self, kind):
        """Multi-device scene: _lib.GATHER_COPY (peer copies, default) or _lib.GATHER_RCCL (grouped ncclSend / ncclRecv)."""
        _check(_lib.lib().sr_set_gather(self._h, int(kind)))

    def rccl_init(self, unique_id, world, rank):
        buf = (C.c_uint8 * _lib.RCCL_ID_BYTES).from_buffer_copy(bytes(unique_id))
        _check(_lib.lib().sr_rccl_init(self._h, buf, int(world), int(rank)))

    def rccl_render(self, frame, d_full_ptr, stream=0):
        """Render this rank's strips of `frame` and gather every rank's on rank 0 (d_full_ptr: device int32[W*H] there, 0 elsewhere)."""
        _check(_lib.lib().sr_rccl_render(self._h, C.byref(frame), C.c_void_p(d_full_ptr) if d_full_ptr else None, C.c_void_p(stream) if stream else None))

    def rccl_gather(self, frame, d_strips_ptr, d_full_ptr, stream=0):
        _check(_lib.lib().sr_rccl_gather(self._h, C.byref(frame), C.c_void_p(d_strips_ptr) if d_strips_ptr else None,
                                         C.c_void_p(d_full_ptr) if d_full_ptr else None, C.c_void_p(stream) if stream else None))


def rccl_unique_id():
    """ncclGetUniqueId through the library (rank 0); hand the 128 bytes to the other ranks."""
    buf = (C.c_uint8 * _lib.RCCL_ID_BYTES)()
    _check(_lib.lib().sr_rccl_unique_id(buf))
    return bytes(buf)


def net_random_jump(seed, skip):
    """The next 55 InternalSample() values of System.Random(seed) after `skip` draws, by the jump-ahead (sr_net_random_jump): int32 [55]."""
    out = np.zeros(55, dtype=np.int32)
    _check(_lib.lib().sr_net_random_jump(int(seed), int(skip), _p(out)))
    return out


def net_random_doubles(seed, n, skip=0):
    """n NextDouble() of System.Random(seed) after `skip` samples."""
    out = np.zeros(int(n))
    _lib.lib().sr_net_random_doubles(int(seed), int(skip), int(n), _p(out))
    return out


def make_random_triangles(n, seed=12345, space=100.0, extent=10.0, origin=0.0, opaque=False):
    """SpatialSubdivisionTests.MakeRandomTriangles with the library's System.Random port."""
    v9 = np.zeros((int(n), 3, 3))
    argb = np.zeros(int(n), dtype=np.uint32)
    _lib.lib().sr_make_random_triangles(int(seed), int(n), float(space), float(extent), float(origin), int(bool(opaque)),
                                        _p(v9), _p(argb))
    return v9, argb


def unit_cube_scene(n, seed=12345):
    """SURVEY 8d synthetic scene (configs 3/4): v1 in [-0.5,0.45]^3, extents U[0,0.05]^3, box [-0.5,0.5]^3."""
    v9, argb = make_random_triangles(n, seed, space=0.95, extent=0.05, origin=-0.5, opaque=True)
    return v9, argb, np.array([-0.5] * 3), np.array([0.5] * 3)


def instance_matrices(position, yaw, pitch, roll):
    pos = np.asarray(position, dtype=np.float64)
    t = np.zeros(12); it = np.zeros(12)
    _lib.lib().sr_instance_matrices(_p(pos), float(yaw), float(pitch), float(roll), _p(t), _p(it))
    return t, it


def default_fov_depth():
    return float(_lib.lib().sr_default_fov_depth())


def area_light_offsets(seed, count=100):
    out = np.zeros((count, 3))
    _lib.lib().sr_area_light_offsets(int(seed), int(count), _p(out))
    return out

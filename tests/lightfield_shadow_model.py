"""CPU model of the colour light field with dynamic soft shadows (rayTraceLightField + rayTraceShadows: LightFieldColorMethod is the outermost
decorator, Renderer.cs:1640-1649, so a cell's canonical ray goes through ShadowMethod and the table stores shadowed colours).  It is
tests/lightfield_model.py with one more step in `fill`, composed only of what the oracle already exports (Scene.trace, area_light_offsets):

  for every canonical ray that hits (ShadowMethod.cs:103-119, 144-179), after shade_points:
    end   = pos + n * 0.001
    point light:        src = L_model + off[i],  ray (src, end - src)       L_model = inv_transform (3 x 4) * light_pos_view
    directional light:  dir = inv_transform (3 x 3) * light_dir_view,  ray (end + dir * 1000.0 + off[i], dir)       (:160-166)
    a ray is blocked iff it hits with ray_frac <= 1.0;  byte = (byte)(escapes / samples * 255);  colour = ModulatePackedColor(colour, byte)

The offset table is made once from the seed (ShadowMethod.cs:63-73) and the step reads only the hit point, the normal and the light: the
shadowed colour of a cell is still a function of the cell alone.
"""
import numpy as np

import ao_model
import lightfield_model as lfm
from helpers import orc

F_SHADOWS = orc.F_SHADOWS
PROBE_OFFSET = 0.001                         # shadowProbeOffset


def shadow_samples_of(f):
    return f.shadow_samples if f.shadow_samples > 0 else 100          # ShadowMethod.cs:9


def light_offsets(f):
    """The frame's offset table: the caller's (sr_frame.area_light_offsets) or the seed's."""
    n = shadow_samples_of(f)
    if f.area_light_offsets:
        import ctypes as C
        return np.ctypeslib.as_array(C.cast(f.area_light_offsets, C.POINTER(C.c_double)), shape=(n, 3)).copy()
    return orc.area_light_offsets(f.random_seed, n)


def light_model(f):
    """(positionalLightPos_Model, directionalLightDir_Model) in the reference's operand order."""
    it = [f.inv_transform[i] for i in range(12)]
    lp, ld = f.light_pos_view, f.light_dir_view
    pos = [lp[0] * it[4 * r] + lp[1] * it[4 * r + 1] + lp[2] * it[4 * r + 2] + it[4 * r + 3] for r in range(3)]
    dirn = [ld[0] * it[4 * r] + ld[1] * it[4 * r + 1] + ld[2] * it[4 * r + 2] for r in range(3)]
    return np.array(pos), np.array(dirn)


def shadow_bytes(scene, f, pos, nrm, target, chunk=20000):
    """ShadowMethod's byte for every surface point (pos, nrm): [n] int64 in 0..255."""
    off = light_offsets(f)
    samples = off.shape[0]
    lpos, ldir = light_model(f)
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    nrm = np.asarray(nrm, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(pos.shape[0], dtype=np.int64)
    for a in range(0, pos.shape[0], chunk):
        end = pos[a:a + chunk] + nrm[a:a + chunk] * PROBE_OFFSET
        if f.flags & orc.F_POINT_LIGHT:
            src = np.broadcast_to((lpos[None, :] + off)[None, :, :], (end.shape[0], samples, 3))
            dirs = end[:, None, :] - src
        else:
            dirs = np.broadcast_to(ldir[None, None, :], (end.shape[0], samples, 3))
            src = (end + ldir[None, :] * 1000.0)[:, None, :] + off[None, :, :]
        res = scene.trace(target, np.ascontiguousarray(src).reshape(-1, 3), np.ascontiguousarray(dirs).reshape(-1, 3))
        blocked = res["hit"].astype(bool) & (res["ray_frac"] <= 1.0)
        escapes = samples - blocked.reshape(-1, samples).sum(axis=1)
        out[a:a + chunk] = (escapes.astype(np.float64) / float(samples) * 255).astype(np.int64) & 255
    return out


class LightFieldShadowModel(lfm.LightFieldModel):
    """One Renderer's LightFieldColorMethod over ShadowMethod: `fill` stores shadowed colours when the frame carries SR_F_SHADOWS."""

    def fill(self, scene, f, index, target):
        u, v, s, t = lfm.decode(index, self.n)
        start = self.points[u, v]
        dirs = self.points[s, t] - start
        res = scene.trace(target, np.ascontiguousarray(start), np.ascontiguousarray(dirs))
        hit = res["hit"].astype(bool)
        col = np.full(index.size, (f.background_argb | 0xFF000000) & 0xFFFFFFFF, dtype=np.uint32)
        if hit.any():
            own = res["color"][hit]
            if f.flags & orc.F_SHADING:
                own = orc.shade_points(f, res["pos"][hit], res["normal"][hit], own)
            if f.flags & F_SHADOWS:
                own = ao_model.modulate(own, shadow_bytes(scene, f, res["pos"][hit], res["normal"][hit], target))
            col[hit] = own
        col[col == 0] = 1
        for i, c in zip(index.tolist(), col.tolist()):
            self.cache[i] = c


def camera_shadow_render(scene, f, target=lfm.TRACE_ROOT_TREE):
    """The frame WITHOUT the light field, its samples shaded and shadowed by the steps `fill` uses: what Scene.render(shadows=True) draws."""
    import pathtrace_model as ptm
    starts, dirs = ptm.camera_samples(f)
    res = scene.trace(target, starts, dirs)
    hit = res["hit"].astype(bool)
    col = np.full(starts.shape[0], (f.background_argb | 0xFF000000) & 0xFFFFFFFF, dtype=np.uint32)
    if hit.any():
        own = res["color"][hit]
        if f.flags & orc.F_SHADING:
            own = orc.shade_points(f, res["pos"][hit], res["normal"][hit], own)
        own = ao_model.modulate(own, shadow_bytes(scene, f, res["pos"][hit], res["normal"][hit], target))
        col[hit] = own
    W, n = f.width, f.sub_pixel_res
    if n == 1:
        return col.reshape(-1, W)
    c = col.reshape(-1, n * n).astype(np.int64)
    r = ((c >> 16) & 255).sum(1) // (n * n)
    g = ((c >> 8) & 255).sum(1) // (n * n)
    bl = (c & 255).sum(1) // (n * n)
    return (0xFF000000 | (r << 16) | (g << 8) | bl).astype(np.uint32).reshape(-1, W)


def shadow_frame(f):
    """`f` with SR_F_SHADOWS OR-ed in."""
    f.flags |= F_SHADOWS
    return f


def gpu_frame(name):
    """(model file, extra geometry, N, frame) of a lfm.GPU_FRAMES entry, with shadows."""
    model, prims, n, f = lfm.gpu_frame(name)
    return model, prims, n, shadow_frame(f)


GOLDEN_NAME = "shading_shadows_lightFieldColor_focalBlurx4"          # RendererTests.RaytraceLightField_Colors (RendererTests.cs:240), the active test


def golden_frame():
    """The frame of the reference's active test: light field, focal blur, shadows, 4 x 4 samples, 100 x 100, N = 64."""
    from helpers import make_frame
    return shadow_frame(lfm.lf_frame(make_frame(100, 100, shading=True, focal_blur=True, sub_pixel_res=4)))


# the frames tests/test_gpu_lightfield_shadows.py renders from lfm.GPU_FRAMES (tests/test_lightfield_shadow_model.py checks their margins)
GPU_FRAME_NAMES = ("view0_n8", "small_blur", "far_primitives", "unit_cube", "inside_sphere")


def gpu_frames():
    """name -> (model file, extra geometry, N, frame): every frame tests/test_gpu_lightfield_shadows.py renders.  Shadows do not move a sample
    into another cell, but the frames' input conditions (lfm.MARGIN) are checked for each of them all the same."""
    out = {"golden": ("obj.3ds", (), 64, golden_frame())}
    for name in GPU_FRAME_NAMES + ("view1_n8", "view2_n8"):
        out[name] = gpu_frame(name)
    for samples in (1, 17, 100, 130):
        model, prims, n, f = gpu_frame("view0_n8")
        f.shadow_samples = samples
        out["samples_%d" % samples] = (model, prims, n, f)
    model, prims, n, f = gpu_frame("view0_n8")
    f.flags &= ~orc.F_POINT_LIGHT
    f.shadow_samples = 17
    out["directional"] = (model, prims, n, f)
    return out

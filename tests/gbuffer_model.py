"""CPU model of the frame G-buffer (sr_render_hits) and of the chain a caller composes over it, made only of what the oracle exports:

  hits     = Scene.trace of pathtrace_model.camera_samples(f): sample ((row - a) * width + col) * n^2 + subX * n + subY
  shading  = oracle shade_points over the hit samples (ShadingMethod's colour step), when SR_F_SHADING is set
  shadows  = shadow_points_model.shadowed over the same samples (ShadowMethod's step), when SR_F_SHADOWS is set
  resolve  = misses keep the background; n^2 samples per pixel are averaged per channel with a truncating divide, alpha 255
             (Renderer.cs:1815-1826); one sample per pixel is the pixel
"""
import numpy as np

import pathtrace_model as ptm
import shadow_points_model as spm
from helpers import orc

KEYS = ("hit", "ray_frac", "pos", "normal", "color", "tri_index")


def hits(scene, f, target):
    """(starts, dirs, Scene.trace's dict) of every camera sample of the frame's rows, in scan order."""
    starts, dirs = ptm.camera_samples(f)
    return starts, dirs, scene.trace(target, starts, dirs)


def background(f):
    return np.uint32((f.background_argb | 0xFF000000) & 0xFFFFFFFF)


def resolve(f, sample_colors):
    """uint32 [rows, width] from one colour per sample in scan order."""
    W, n = f.width, f.sub_pixel_res
    col = np.asarray(sample_colors, dtype=np.uint32)
    if n == 1:
        return col.reshape(-1, W)
    c = col.reshape(-1, n * n).astype(np.int64)
    r = ((c >> 16) & 255).sum(1) // (n * n)
    g = ((c >> 8) & 255).sum(1) // (n * n)
    b = (c & 255).sum(1) // (n * n)
    return (0xFF000000 | (r << 16) | (g << 8) | b).astype(np.uint32).reshape(-1, W)


def compose(scene, f, target):
    """The frame as the chain over the G-buffer gives it: uint32 [rows, width]."""
    _, _, res = hits(scene, f, target)
    hit = res["hit"].astype(bool)
    col = np.full(hit.size, background(f), dtype=np.uint32)
    pos, nrm, own = res["pos"][hit], res["normal"][hit], res["color"][hit]
    if f.flags & orc.F_SHADING:
        own = orc.shade_points(f, pos, nrm, own)
    if f.flags & orc.F_SHADOWS:
        own = spm.shadowed(scene, f, pos, nrm, own, target)
    col[hit] = own
    return resolve(f, col)

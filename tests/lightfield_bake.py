"""What the tests of sr_bake_light_field share: the whole table of a scene as the CPU model (tests/lightfield_model.py) fills it -- every
cell's canonical ray through LightFieldModel.fill -- the frames the bakes use, and the figures of those tables that the tests stand on
(recomputed by tests/test_lightfield_bake_model.py without a GPU)."""
import numpy as np

import lightfield_model as lfm
from helpers import load_obj3ds, make_frame, orc, unit_cube_scene

BACKGROUND = 0xFFFF00FF                      # make_frame's background with the alpha a stored colour carries

# (model, N) -> (entries that are not the background, entries): the same with and without shading
NON_BACKGROUND = {("obj.3ds", 2): (24, 64), ("obj.3ds", 4): (194, 1024), ("obj.3ds", 8): (3804, 16384), ("obj.3ds", 12): (19166, 82944),
                  ("unit_cube_2000", 8): (1842, 16384), ("unit_cube_2000", 16): (29401, 262144)}


def bake_frame(shading=True, **kw):
    """A light-field frame whose camera fields do not matter to a bake: 16 x 16, the reference's regression pose unless `kw` says otherwise."""
    return lfm.lf_frame(make_frame(16, shading=shading, **kw))


def oracle_scene(model, prims=()):
    o = orc.Scene()
    o.set_triangles(*(unit_cube_scene(2000) if model == "unit_cube_2000" else load_obj3ds(model)))
    if prims:
        o.set_extra(list(prims))
    assert o.build_tree() == 0
    return o


def model_entries(o, f, n, index, target):
    """The model's colours of the cells `index` (any order, no duplicates) from an empty cache."""
    m = lfm.LightFieldModel(n)
    index = np.asarray(index, dtype=np.int64)
    m.fill(o, f, index, target)
    return m.entries(index)


def model_table(o, f, n, target):
    """All 4 N^4 entries: what a bake of an empty table must leave."""
    return model_entries(o, f, n, np.arange(lfm.cache_entries(n), dtype=np.int64), target)


def diagonal_cells(n):
    """The cells (u, v, u, v): their canonical direction is the zero vector."""
    u, v = np.meshgrid(np.arange(2 * n), np.arange(n), indexing="ij")
    u, v = u.reshape(-1), v.reshape(-1)
    return u * n * n * n * 2 + v * n * n * 2 + u * n + v

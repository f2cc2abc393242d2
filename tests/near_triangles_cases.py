"""Scenes, points and radii of the sr_near_triangles tests (tests/test_gpu_near_triangles.py), shared with tests/test_near_triangles_model.py,
which pins on the CPU what they hold.  The scenes and point sets are the closest-point tests' own (tests/closest_points_cases.py, imported
and not edited); K takes the values of KS.
Radii: radius_kinds rotates ten kinds over the points, around every point's own neighbours in the model: +inf, 0, the nearest distance, the
exact distance of the 4th neighbour, one ulp below it, NaN, -inf, -1, 1/8 of the largest box extent, twice the nearest distance.
model(scene) answers the scene's points once -- without a limit ("none"), under the rotating radii ("radii") and, counts only, under the
radius extent / 8 for every point ("extent8") -- and is left unchanged."""
import functools

import numpy as np

import closest_points_cases as cpc
import near_triangles_model as ntm

SCENES = cpc.SCENES
KS = (0, 1, 4, 64)
RADIUS_KINDS = ("inf", "zero", "nearest", "fourth", "below_fourth", "nan", "-inf", "negative", "extent8", "double")


def extent8(name):
    _, _, bmin, bmax = cpc.scene(name)
    return float((bmax - bmin).max()) / 8.0


def radius_kinds(first, nearest, fourth, ext8):
    """([p] radii, [p] kind index into RADIUS_KINDS) for the points first .. first + p - 1 with the given nearest and 4th-neighbour distances."""
    nearest = np.asarray(nearest, dtype=np.float64)
    fourth = np.asarray(fourth, dtype=np.float64)
    p = nearest.shape[0]
    kind = (first + np.arange(p)) % len(RADIUS_KINDS)
    table = np.stack([np.full(p, np.inf), np.zeros(p), nearest, fourth, np.nextafter(fourth, -np.inf), np.full(p, np.nan), np.full(p, -np.inf),
                      np.full(p, -1.0), np.full(p, ext8), nearest * 2.0])
    return np.ascontiguousarray(table[kind, np.arange(p)]), kind


class Model:
    """sets: {"none", "radii": near_triangles_model.Rows; "extent8": its counts [P]}; limits: {"radii", "extent8": [P]}; kind [P]; nan_pairs [P]."""

    def __init__(self, name):
        self.name = name
        self.points = cpc.points(name)
        v9 = cpc.scene(name)[0]
        P = self.points.shape[0]
        ext8 = extent8(name)
        self.limits = {"radii": np.zeros(P), "extent8": np.full(P, ext8)}
        self.kind = np.zeros(P, dtype=np.int64)

        def make(first, block):
            lim, kind = radius_kinds(first, block.dist[:, 0], block.dist[:, 3], ext8)
            self.limits["radii"][first:first + lim.shape[0]] = lim
            self.kind[first:first + lim.shape[0]] = kind
            return {"radii": lim, "extent8": np.full(lim.shape[0], ext8)}

        made = ntm.near_sets(self.points, v9, make)
        self.nan_pairs = made["nan_pairs"]
        self.sets = {"none": made["none"], "radii": made["radii"], "extent8": made["extent8"].count}
        for a in (self.nan_pairs, self.kind, self.sets["extent8"], *self.limits.values()):
            a.setflags(write=False)
        for rows in (self.sets["none"], self.sets["radii"]):
            for k in ("count", "index", "d2", "dist", "pos", "uv"):
                getattr(rows, k).setflags(write=False)

    def want(self, which, k):
        return self.sets[which].rows(k)

    def limit(self, which):
        return None if which == "none" else self.limits[which]


@functools.lru_cache(maxsize=None)
def model(name):
    return Model(name)

"""The model of sr_nearest_rays, shared by tests/test_nearest_rays_model.py (CPU, against the oracle) and tests/test_gpu_nearest_rays.py: the
answer of a trace() -- the library's or the oracle's -- with every hit whose ray_frac exceeds its ray's limit blanked to trace()'s miss (hit 0,
zeros, tri_index -1).  The comparison is IEEE <=: a NaN limit and a negative one blank every hit, +inf none; limits None is no limit.
Scenes, ray sets and limits are those of tests/occluded_rays_cases.py, unchanged."""
import numpy as np

KEYS = ("hit", "ray_frac", "pos", "normal", "color", "tri_index")


def nearest_model(res, limits):
    """dict with KEYS from an answer of trace() and the limits ([n] or None)."""
    out = {k: np.array(res[k], copy=True) for k in KEYS}
    if limits is None:
        return out
    hit = np.asarray(res["hit"]).astype(bool)
    with np.errstate(invalid="ignore"):
        keep = hit & (np.asarray(res["ray_frac"]) <= np.asarray(limits, dtype=np.float64))
    cut = ~keep
    out["hit"][cut] = 0
    out["ray_frac"][cut] = 0.0
    out["pos"][cut] = 0.0
    out["normal"][cut] = 0.0
    out["color"][cut] = 0
    out["tri_index"][cut] = -1
    return out


def shares(res, limits):
    """(kept, cut, miss) counts of an answer of trace() under the limits."""
    hit = np.asarray(res["hit"]).astype(bool)
    with np.errstate(invalid="ignore"):
        keep = hit & (np.asarray(res["ray_frac"]) <= limits)
    return int(keep.sum()), int((hit & ~keep).sum()), int((~hit).sum())


def same_bits(got, want, keys=KEYS):
    """Every key of `keys` equal bit for bit (a -0.0 is not a 0.0), same shapes, same item sizes."""
    for k in keys:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.dtype.itemsize != b.dtype.itemsize or a.tobytes() != b.tobytes():
            return False
    return True


def same_values(got, want, keys=KEYS):
    """Every key equal by value (the oracle's arrays have dtypes of their own)."""
    return all(np.asarray(got[k]).shape == np.asarray(want[k]).shape and np.array_equal(np.asarray(got[k]), np.asarray(want[k])) for k in keys)


def take(res, mask, keys=KEYS):
    return {k: np.asarray(res[k])[mask] for k in keys}

"""Expected values of the geometry channels of the `aov` integrator (dtof_sample_aov_lanes, dtof_render_aovs), from the oracle alone: nothing here touches the
library under test.

  lanes     sample_pos, time, ray_o, ray_d of every lane from orc.Scene.render_lanes (moments_ref.lanes_of): the scene integrator's own lanes
  values    per lane orc_kat_ray_intersect(scene, o, d, time, FLT_MAX, out25, ids): t, p, n, sh_n, sh_s, sh_t, dp_du, dp_dv, wi and (object, shape, prim).  A miss is
            all zeros; prim_index is (float) ids[2].  The call has no far plane, so every test that uses these values asserts on the ORACLE's numbers that
            (a) every hit has t < far_clip - near_clip, a lower bound of every camera ray's maxt (maxt = (far_clip - near_clip) / cos >= far_clip - near_clip), and,
            where the scene is open, (b) that hits and misses both occur.
  uv, shape_index   the oracle's record has neither.  Their columns in `values` are NaN on a hit (0 on a miss, which IS known): the per-lane tests check them by
            other means (the device's pinned ray query, the closed form of a rectangle, the structure of the oracle's (object, shape) ids), and the film tests fill
            them with the per-lane entry's output, which those tests pin.
  films     moments_ref.footprint / moments_ref.splat over the lane values, column 0 the value 1: float32 terms value * (wx * wy), summed in float64
"""
import ctypes as C

import numpy as np

import moments_ref as ref

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
TYPES = ("depth", "position", "uv", "geo_normal", "sh_normal", "dp_du", "dp_dv", "prim_index", "shape_index")
CHANNELS = {"depth": ["T"], "position": ["X", "Y", "Z"], "uv": ["U", "V"], "geo_normal": ["X", "Y", "Z"], "sh_normal": ["X", "Y", "Z"], "dp_du": ["X", "Y", "Z"],
            "dp_dv": ["X", "Y", "Z"], "prim_index": ["I"], "shape_index": ["I"]}
ALL_NINE = "d:depth,p:position,u:uv,g:geo_normal,s:sh_normal,a:dp_du,b:dp_dv,i:prim_index,h:shape_index"      # C = 20
# columns of out25 per type (None: not in the oracle's record)
_OUT25 = {"depth": [0], "position": [1, 2, 3], "uv": None, "geo_normal": [4, 5, 6], "sh_normal": [7, 8, 9], "dp_du": [16, 17, 18], "dp_dv": [19, 20, 21],
          "prim_index": "prim", "shape_index": None}


def parse(spec):
    """[(name, type)] of a well-formed spec, split as string::tokenize splits it"""
    items = []
    for token in spec.replace(" ", ",").split(","):
        if token:
            name, typ = [p for p in token.split(":") if p]
            items.append((name, typ))
    return items


def channel_names(spec):
    return ["%s.%s" % (name, sfx) for name, typ in parse(spec) for sfx in CHANNELS[typ]]


def intersect(orc, osc, lanes):
    """orc_kat_ray_intersect per lane -> (out25 (N, 25) float32, ids (N, 3) int32)"""
    L = orc.lib()
    n = len(lanes)
    out, ids = np.zeros((n, 25), F32), np.zeros((n, 3), np.int32)
    o, d, t = np.ascontiguousarray(lanes["ray_o"], F32), np.ascontiguousarray(lanes["ray_d"], F32), np.ascontiguousarray(lanes["time"], F32)
    for i in range(n):
        L.orc_kat_ray_intersect(C.byref(osc.c), o[i].ctypes.data, d[i].ctypes.data, float(t[i]), FLT_MAX, out[i].ctypes.data, ids[i].ctypes.data)
    return out, ids


def check_far_plane(osc, out25, ids):
    """condition (a), on the oracle's numbers"""
    se = osc.flat.sensor
    hit = ids[:, 0] >= 0
    limit = F32(se["far_clip"]) - F32(se["near_clip"])
    assert hit.any() and (out25[hit, 0] < limit).all(), "an oracle hit lies beyond far_clip - near_clip: the oracle's query has no far plane"
    return hit


def lane_values(spec, out25, ids):
    """(N, C) float32 in channel order; NaN where the oracle's record has no value (uv and shape_index of a hit)"""
    hit = ids[:, 0] >= 0
    cols = []
    for _, typ in parse(spec):
        src = _OUT25[typ]
        if src is None:
            cols += [np.where(hit, F32(np.nan), F32(0))] * len(CHANNELS[typ])
        elif src == "prim":
            cols.append(np.where(hit, ids[:, 2].astype(F32), F32(0)))
        else:
            cols += [np.where(hit, out25[:, k], F32(0)) for k in src]
    return np.stack(cols, axis=1).astype(F32)


def shape_records(osc, ids):
    """the shape record every oracle hit lies on (its index in the oracle's own shape table, -1 on a miss): an object that is a shape names its record, an
    instance the record `shape` of its group"""
    fs = osc.flat
    rec = np.full(len(ids), -1, np.int64)
    for i, (ob, sh, _) in enumerate(ids):
        if ob >= 0:
            o = fs.objects[ob]
            rec[i] = o["index"] if o["kind"] == 0 else fs.groups[o["index"]]["first_shape"] + sh
    return rec


def expected_lanes(orc, osc, spec, seed, spp, override=None):
    """(lanes of the render, values (N, C), out25, ids) with the far-plane condition asserted"""
    pd = osc.params(integrator=override) if override else osc.params()
    lanes = ref.lanes_of(orc, osc, pd, seed, spp)
    out25, ids = intersect(orc, osc, lanes)
    check_far_plane(osc, out25, ids)
    return lanes, lane_values(spec, out25, ids), out25, ids, pd


def expected_planes(orc, osc, lanes, values, pd, spp):
    """the raw planes (1 + C, H, W) of one render and the sums of the terms' magnitudes; `values` without NaNs"""
    assert np.isfinite(values).all()
    spw, _ = ref.pass_layout(orc, osc, pd, spp)
    fp = ref.footprint(orc, osc, lanes["sample_pos"], spw)
    cols = np.concatenate([np.ones((len(values), 1), F32), values], axis=1)
    return ref.splat(osc, fp, cols)


def errors_over_bound(got, want, mags):
    return ref.errors_over_bound(got, want, mags)

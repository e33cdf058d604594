"""Scenes and ray families of the flat-table sweep (test_flat_sweep_cpu.py, test_flat_sweep_gpu.py): the ray query of the fused kernels of flat scenes -- trace_flat
(mitsuba3dopplertof_amd/csrc/dtof_traverse.h) in its three forms, through dtof_flat_query -- against the oracle's scene_closest / scene_occluded over the same rays
(orc_kat_flat_n, which also reports the operands of every compare of every rectangle: the local z of origin and direction, t, u, v, the best t at the visit).

Scenes, all derived from scenes/cornell_wall.xml (five rectangles, the moving back wall an instance at index 2); `forms` are the forms of dtof_flat_query a scene meets:

  closed         cornell_wall as it is                                                         generic, one_wall, shape
  panel          the left wall a free-standing panel (tests/test_flat_shape.py): shadowed rays   generic, one_wall, shape
  ties_wall      five rectangles, the wall at index 2: floor, ceiling, wall, A SECOND FLOOR, a plain rectangle in the wall's start pose.  The one-wall variant of
                 `ties` the three forms can all run: two plain rectangles that tie at every ray, and the wall against a plain rectangle at time 0.  It is an open
                 room (no side walls), so `closed` stays what it is next to it: a closed room with a tie is not possible with five rectangles and the wall at index 2
                 (floor, ceiling, back, right and left wall take all five).                    generic, one_wall, shape
  wall_at_3      the wall moved to index 3                                                     generic, one_wall
  six            a sixth, tilted rectangle                                                     generic, one_wall
  no_instance    the wall made static: five plain rectangles                                   generic
  two_instances  the back wall's group holds two rectangles, the left wall moves as well        generic (the instances loop through intersect_object)
  eight          kFlatObjects objects                                                          generic
  one            the floor alone                                                               generic
  ties           closed + a second floor + a plain rectangle in the wall's start pose          generic

Ray families (the letter is a ray's label; every ray serves both query kinds):

  A   random: origins in the room's box and a little outside, directions uniform on the sphere, times over the shutter and its two ends, maxt inf / the largest float /
      random finite.  A2: rays THROUGH two rectangles, from behind one towards a point of another, so that a rectangle is met behind a nearer hit (t > best).
  B   edges: for every rectangle, rays across each of its four edges and towards its four corners; one component of the direction is bisected ON THE ORACLE to the
      last float with |u| <= 1 (or |v| <= 1) and its neighbour, and issued a few floats either side.
  C   maxt: every (ray, rectangle) of the other families whose t, u, v pass, again with maxt the float below t, t itself and the float above, and with maxt either side
      of t / (1 + 2^-20), where flat_cull_far(maxt) crosses t.  C2: maxt = 0, -0, the
      smallest denormal, 2^-100, -1 on rays that start in a rectangle's plane and on random ones.
  D   in the plane: origins bisected on the oracle to the two floats where the local z of the origin changes sign (exactly 0 where a float achieves it), a float either
      side, directions towards the plane and away from it.  D2: the same origins with directions of length 1e30 and 1e38: t = -zx / zy underflows to +-0 for ANY
      rectangle.  S: shadow-ray-like segments between two points, maxt = dist * (1 - kShadowEps) as k_shade forms it, half of them starting on a rectangle.
  E   parallel: directions whose local z is +-0 or a few denormals (directions of denormal length), and directions in the rectangle's plane with one component bisected
      to the sign change of the local z; origins off the plane and in it (0 / 0 where D found an exact zero).
  F   ties (the two scenes with doubled rectangles): rays aimed at the doubled rectangles.
  G   the wall: rays aimed at and around every instance's rectangles, each at two times; and with maxt between the two hit distances (a hit at one time only).  The
      wall's own space is not the world's (the instance matrix is the whole pose), so every one of them distinguishes the wall's ray from the world's.
  H   non-finite and extreme: NaN / +-inf in each component of origin and direction in turn, maxt NaN / -inf, a zero direction, origins at 1e30 with directions of
      length 1, 1e-30, 1e30.  None of them hits.  HT: time NaN / +-inf (the keyframe weight clamps: plain rectangles are hit as ever).  X: directions of length
      1e-30, 1e30, 1e38 and denormal from ordinary origins.
  M   certain misses: rays far in front of the room that fly away from it with a finite maxt; flat_certain_miss settles every rectangle for them.

Placements: the families in order (homogeneous waves), one fixed permutation (mixed waves), and short lists of 1, 63, 64, 65 rays cut from M with ONE other ray: a ray
that hits, or a ray of C ON a bound (t == maxt, t == 0) -- a lane whose full test no neighbour asks for.
Everything is a function of SEED."""
import ctypes as C
import os
import re

import numpy as np

from conftest import SCENES

F32 = np.float32
SEED = 20260419
SHUTTER = 0.0015
INF = F32(np.inf)
FMAX = np.finfo(np.float32).max
SHADOW_EPS = F32(F32(1500.0) * F32(5.9604644775390625e-8)) * F32(10.0)      # kShadowEps (dtof_math.h): kRayEps * 10
ZX, ZY, T, U, V, BEST = range(6)                                             # ORC_FLAT_* (oracle/dtof_oracle.h)
CANARY = 0x7fc0beef
FORMS = ("generic", "one_wall", "shape")
KINDS = ("closest", "occlusion")
SCENE_FORMS = [("closed", (0, 1, 2)), ("panel", (0, 1, 2)), ("ties_wall", (0, 1, 2)), ("wall_at_3", (0, 1)), ("six", (0, 1)), ("no_instance", (0,)),
               ("two_instances", (0,)), ("eight", (0,)), ("one", (0,)), ("ties", (0,))]
NAMES = [n for n, _ in SCENE_FORMS]
CASES = [(n, f, k) for n, forms in SCENE_FORMS for f in forms for k in KINDS]
TIE_SCENES = ("ties", "ties_wall")

SHAPE_BLOCK = r'\t<shape type="rectangle" id="%s">.*?</shape>\n'
# (tests/test_flat_shape.py) a rectangle of side 0.6 that faces the camera, in front of the back wall and above the floor; a tilted sixth rectangle
PANEL = ('\t<shape type="rectangle" id="LeftWall">\n\t\t<transform name="to_world"><scale value="0.3" /><translate x="0.3" y="0.6" z="0.2" /></transform>\n'
         '\t\t<ref id="LeftWallBSDF" />\n\t</shape>\n')
SIXTH = ('\t<shape type="rectangle" id="Tilted"><transform name="to_world"><scale x="0.3" y="0.7" z="1" /><rotate x="0.3" y="1" z="0.2" angle="37" />'
         '<translate x="0.2" y="0.9" z="0.1" /></transform><ref id="ShortBoxBSDF" /></shape>\n')
SEVENTH = ('\t<shape type="rectangle" id="Low"><transform name="to_world"><scale x="0.5" y="0.25" z="1" /><rotate x="1" angle="-70" />'
           '<translate x="-0.4" y="0.3" z="0.4" /></transform><ref id="TallBoxBSDF" /></shape>\n')
EIGHTH = ('\t<shape type="rectangle" id="Slab"><transform name="to_world"><scale x="0.4" y="0.4" z="1" /><rotate y="1" angle="90" />'
          '<translate x="0.5" y="1.4" z="-0.3" /></transform><ref id="TallBoxBSDF" /></shape>\n')
INNER = ('\t\t<shape type="rectangle"><transform name="to_world"><scale x="0.25" y="0.5" z="1" /><translate x="0.3" y="-0.2" z="0.35" /></transform>'
         '<ref id="ShortBoxBSDF" /></shape>\n')


def scene_xml(name):
    """the scene `name` as an XML string"""
    xml = open(os.path.join(SCENES, "cornell_wall.xml")).read()
    block = {k: re.search(SHAPE_BLOCK % k, xml, re.S).group(0) for k in ("Floor", "Ceiling", "BackWall", "RightWall", "LeftWall")}
    key0 = re.search(r'<transform time="0">\s*(<matrix value="[^"]*" />)', block["BackWall"]).group(1)
    static_wall = '\t<shape type="rectangle" id="%s">\n\t\t<transform name="to_world">\n\t\t\t' + key0 + '\n\t\t</transform>\n\t\t<ref id="BackWallBSDF" />\n\t</shape>\n'
    second_floor = block["Floor"].replace('id="Floor"', 'id="Floor2"')
    before_emitter = lambda s, extra: s.replace("\t<emitter", extra + "\t<emitter", 1)      # noqa: E731
    if name == "closed":
        return xml
    if name == "panel":
        return xml.replace(block["LeftWall"], PANEL)
    if name == "wall_at_3":
        return xml.replace(block["BackWall"], "").replace(block["RightWall"], block["RightWall"] + block["BackWall"])
    if name == "six":
        return before_emitter(xml, SIXTH)
    if name == "eight":
        return before_emitter(xml, SIXTH + SEVENTH + EIGHTH)
    if name == "no_instance":
        return xml.replace(block["BackWall"], static_wall % "BackWall")
    if name == "one":
        for k in ("Ceiling", "BackWall", "RightWall", "LeftWall"):
            xml = xml.replace(block[k], "")
        return xml
    if name == "ties":
        return before_emitter(xml, second_floor + static_wall % "WallPose")
    if name == "ties_wall":
        return xml.replace(block["RightWall"], second_floor).replace(block["LeftWall"], static_wall % "WallPose")
    if name == "two_instances":
        anim = re.search(r"<animation name=\"to_world\">.*?</animation>", block["BackWall"], re.S).group(0)
        group = ('\t<shape type="shapegroup" id="BackGroup">\n\t\t<shape type="rectangle"><ref id="BackWallBSDF" /></shape>\n' + INNER + '\t</shape>\n'
                 '\t<shape type="instance">\n\t\t<ref id="BackGroup" />\n\t\t' + anim + '\n\t</shape>\n')
        left = re.search(r'<matrix value="[^"]*" />', block["LeftWall"]).group(0)
        moving_left = ('\t<shape type="rectangle" id="LeftWall">\n\t\t<animation name="to_world">\n\t\t\t<transform time="0">' + left + '</transform>\n'
                       '\t\t\t<transform time="0.0015">' + left + '<translate x="0.01" y="0.0" z="0.0" /></transform>\n\t\t</animation>\n\t\t<ref id="LeftWallBSDF" />\n\t</shape>\n')
        return xml.replace(block["BackWall"], group).replace(block["LeftWall"], moving_left)
    raise KeyError(name)


# ---------------------------------------------------------------------------- floats as ordered integers
def ordf(x):
    i = np.ascontiguousarray(x, F32).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, -(i & 0x7fffffff))


def unordf(o):
    o = np.asarray(o, np.int64)
    return np.where(o >= 0, o, (-o) | 0x80000000).astype(np.uint32).view(F32)


def step(x, k):
    """the float k floats above x (below for k < 0)"""
    return unordf(ordf(x) + k)


def bisect(pred, lo, hi):
    """pred(lo) holds, pred(hi) does not (elementwise, float32): -> (lo, hi) ADJACENT floats with the same property; pred sees whole arrays"""
    lo, hi = ordf(lo), ordf(hi)
    while (np.abs(hi - lo) > 1).any():
        mid = (lo + hi) // 2
        p = pred(unordf(mid))
        lo, hi = np.where(p, mid, lo), np.where(p, hi, mid)
    return unordf(lo), unordf(hi)


def rays8(o, d, time, maxt):
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    n = max(len(o), len(d))
    r = np.zeros((n, 8), F32)
    with np.errstate(over="ignore", invalid="ignore"):
        r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7] = o, d, time, maxt
    return r


# ---------------------------------------------------------------------------- the rectangles of a scene, in the oracle's visit order
class Geometry:
    """slot r = the r-th rectangle the oracle visits: its object, its shape's local -> world matrix (the inverse of the to_object the rectangle test reads: a loader's
    to_world need not be its exact inverse) and, for a member of an instance's group, the instance's keyframes"""

    def __init__(self, osc):
        fs = osc.flat
        self.slots = []
        for oi, ob in enumerate(fs.objects):
            if ob["kind"] == 0:
                self.slots.append((oi, np.linalg.inv(np.asarray(fs.shapes[ob["index"]]["to_object"], np.float64)), None))
            else:
                g = fs.groups[ob["index"]]
                for k in range(g["n_shapes"]):
                    self.slots.append((oi, np.linalg.inv(np.asarray(fs.shapes[g["first_shape"] + k]["to_object"], np.float64)), ob))
        self.n = len(self.slots)
        self.instances = [r for r, s in enumerate(self.slots) if s[2] is not None]

    def matrices(self, r, time):
        """(n, 4, 4) local -> world of slot r at the times `time`"""
        oi, s2w, ob = self.slots[r]
        time = np.atleast_1d(np.asarray(time, np.float64))
        if ob is None:
            return np.broadcast_to(s2w, (len(time), 4, 4))
        k0, k1 = np.asarray(ob["key"][0], np.float64), np.asarray(ob["key"][1], np.float64)
        if ob["n_keys"] <= 1:
            return np.broadcast_to(k0 @ s2w, (len(time), 4, 4))
        a = np.clip((time - float(ob["key_time"][0])) / (float(ob["key_time"][1]) - float(ob["key_time"][0])), 0, 1)[:, None, None]
        return (k0 * (1 - a) + k1 * a) @ s2w

    def point(self, r, u, v, time):
        u, v = np.atleast_1d(u), np.atleast_1d(v)
        p = np.stack([u, v, np.zeros_like(u), np.ones_like(u)], 1)
        return np.einsum("nij,nj->ni", self.matrices(r, time if np.ndim(time) else np.full(len(u), time)), p)[:, :3]

    def axes(self, r, time=0.0):
        """world directions of the local u, v and normal axes of slot r"""
        m = self.matrices(r, time)[0]
        return m[:3, 0], m[:3, 1], m[:3, 2]


def _sphere(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _times(rng, n):
    t = rng.uniform(0, SHUTTER, n)
    t[0::5] = 0.0
    t[1::5] = SHUTTER
    return t


def _inside(rng, n, shrink=0.8):
    return np.stack([rng.uniform(-shrink, shrink, n), rng.uniform(1 - shrink, 1 + shrink, n), rng.uniform(-shrink, shrink, n)], 1)


def _maxts(rng, n):
    m = rng.uniform(0.0, 4.0, n)
    pick = rng.integers(0, 3, n)
    return np.where(pick == 0, np.inf, np.where(pick == 1, float(FMAX), m))


def passes(ops, maxt=None):
    """(n, slots) bool: t >= 0, |u| <= 1, |v| <= 1 (and t <= maxt if given) of every rectangle"""
    with np.errstate(invalid="ignore"):
        ok = (ops[..., T] >= 0) & (np.abs(ops[..., U]) <= 1) & (np.abs(ops[..., V]) <= 1)
        return ok & (ops[..., T] <= np.asarray(maxt, F32)[:, None]) if maxt is not None else ok


class Sweep:
    """the rays of one scene with their labels, placements and oracle answers"""

    def __init__(self, name, orc, n_random=3000):
        self.name, self.forms = name, dict(SCENE_FORMS)[name]
        self.xml = scene_xml(name)
        self.osc = orc.Scene(self.xml, dict(resx=16, resy=16), is_string=True)
        self.geo = Geometry(self.osc)
        self.parts = []
        rng = np.random.default_rng([SEED, NAMES.index(name)])
        self._random(rng, n_random)
        self._edges(rng)
        self._plane(rng)
        self._parallel(rng)
        if name in TIE_SCENES:
            self._ties(rng)
        self._wall(rng)
        self._extreme(rng)
        self._misses(rng)
        self._maxt(rng)      # (last: it repeats rays of the families before it)
        self.rays = np.ascontiguousarray(np.concatenate([r for _, r in self.parts]))
        self.family = np.concatenate([np.full(len(r), f, dtype="U2") for f, r in self.parts])
        self.n = len(self.rays)
        self.perm = np.random.default_rng([SEED, 99]).permutation(self.n)
        self.want = self.osc.flat_n(self.rays)
        self.finite = np.isfinite(self.rays[:, :7]).all(axis=1) & ~np.isnan(self.rays[:, 7])
        self._short_lists()

    def oracle(self, rays, operands=True):
        return self.osc.flat_n(rays, operands)

    def add(self, family, rays):
        if len(rays):
            self.parts.append((family, np.ascontiguousarray(rays, F32).reshape(-1, 8)))

    def of(self, *families):
        return np.concatenate([r for f, r in self.parts if f in families])

    # ---- A
    def _random(self, rng, n):
        o = np.stack([rng.uniform(-1.3, 1.3, n), rng.uniform(-0.3, 2.3, n), rng.uniform(-1.3, 1.6, n)], 1)
        self.add("A", rays8(o, _sphere(rng, n), _times(rng, n), _maxts(rng, n)))
        g, through = self.geo, []
        for j in range(g.n):
            for k in range(g.n):
                if j != k:
                    m = 40
                    tm = _times(rng, m)
                    p, q = g.point(j, rng.uniform(-.9, .9, m), rng.uniform(-.9, .9, m), tm), g.point(k, rng.uniform(-.9, .9, m), rng.uniform(-.9, .9, m), tm)
                    through.append(rays8(p - 0.25 * (q - p), q - p, tm, np.where(rng.integers(0, 2, m) == 0, np.inf, 3.0)))
        if through:
            self.add("A2", np.concatenate(through))

    # ---- B
    def _edges(self, rng, per_feature=4):
        g = self.geo
        o_all, d_all, ax_all, xin, xout, slot, coord, tm_all = [], [], [], [], [], [], [], []
        for r in range(g.n):
            feats = [(c, s, None) for c in (U, V) for s in (-1, 1)] + [(c, s, s2) for c in (U, V) for s in (-1, 1) for s2 in (-1, 1)]      # edges; corners, bisected along u and along v
            for c, s, s2 in feats:
                m = per_feature
                tm = _times(rng, m)
                other = rng.uniform(-0.8, 0.8, m) if s2 is None else np.full(m, s2 * 0.999999)
                uv_in = (np.full(m, s * 0.97), other) if c == U else (other, np.full(m, s * 0.97))
                uv_out = (np.full(m, s * 1.3), other) if c == U else (other, np.full(m, s * 1.3))
                o = _inside(rng, m)
                d_in, d_out = (g.point(r, *uv_in, tm) - o).astype(F32), (g.point(r, *uv_out, tm) - o).astype(F32)
                e = g.axes(r)[0 if c == U else 1]
                ax = int(np.argmax(np.abs(e)))
                o_all.append(o); d_all.append(d_in); ax_all += [ax] * m; xin.append(d_in[:, ax]); xout.append(d_out[:, ax]); slot += [r] * m; coord += [c] * m; tm_all.append(tm)
        o, d, tm = np.concatenate(o_all).astype(F32), np.concatenate(d_all), np.concatenate(tm_all).astype(F32)
        ax, slot, coord, xin, xout = np.array(ax_all), np.array(slot), np.array(coord), np.concatenate(xin), np.concatenate(xout)
        idx = np.arange(len(o))

        def make(x, keep=slice(None)):
            dd = d[keep].copy()
            dd[np.arange(len(dd)), ax[keep]] = x
            return rays8(o[keep], dd, tm[keep], np.inf)

        def inside(x, keep=slice(None)):
            ops = self.oracle(make(x, keep))["ops"]
            k = idx[keep]
            with np.errstate(invalid="ignore"):
                return np.abs(ops[np.arange(len(k)), slot[k], coord[k]]) <= 1
        keep = inside(xin) & ~inside(xout)
        lo, hi = bisect(lambda x: inside(x, keep), xin[keep], xout[keep])
        toward = np.sign(ordf(hi) - ordf(lo))
        back = [make(x, keep) for x in (lo, hi)]      # ... and the two boundary rays flown backwards: t < 0 beside |u| = 1
        for y in back:
            y[:, 3:6] = -y[:, 3:6]
        self.add("B", np.concatenate([make(unordf(ordf(lo) + toward * k), keep) for k in range(-3, 5)] + back))

    # ---- D, D2, S
    def _plane(self, rng, per_rect=12):
        g = self.geo
        o_all, ax_all, slot, tm_all, nrm = [], [], [], [], []
        for r in range(g.n):
            m = per_rect
            u = np.concatenate([[0, .5, .125, -.25], rng.uniform(-.9, .9, m - 4)])
            v = np.concatenate([[0, .25, -.25, .5], rng.uniform(-.9, .9, m - 4)])
            tm = _times(rng, m)
            n = g.axes(r)[2]
            o_all.append(g.point(r, u, v, tm)); ax_all += [int(np.argmax(np.abs(n)))] * m; slot += [r] * m; tm_all.append(tm); nrm += [n / np.linalg.norm(n)] * m
        o, tm, ax, slot, nrm = np.concatenate(o_all).astype(F32), np.concatenate(tm_all).astype(F32), np.array(ax_all), np.array(slot), np.array(nrm)
        some_d = np.ones((len(o), 3))

        def zx(x, keep=slice(None)):
            oo = o[keep].copy()
            oo[np.arange(len(oo)), ax[keep]] = x
            return self.oracle(rays8(oo, some_d[keep], tm[keep], np.inf))["ops"][np.arange(len(oo)), slot[keep], ZX]
        x0 = o[np.arange(len(o)), ax]
        xa, xb = (x0 - F32(0.01)).astype(F32), (x0 + F32(0.01)).astype(F32)
        za, zb = zx(xa), zx(xb)
        keep = np.sign(za) * np.sign(zb) < 0
        sa = np.sign(za[keep])
        lo, hi = bisect(lambda x: zx(x, keep) * sa > 0, xa[keep], xb[keep])
        toward = np.sign(ordf(hi) - ordf(lo))
        rays, huge, self.plane_origins = [], [], []
        for k in (-1, 0, 1, 2):      # lo - 1, lo, hi (zx == 0 where a float achieves it, else the first float beyond), hi + 1
            oo = o[keep].copy()
            oo[np.arange(len(oo)), ax[keep]] = unordf(ordf(lo) + toward * k)
            self.plane_origins.append((oo, tm[keep], slot[keep]))
            for sgn in (-1, 1):
                for tilt in (0.0, 0.6):
                    d = sgn * nrm[keep] + tilt * _sphere(rng, len(oo))
                    rays.append(rays8(oo, d, tm[keep], np.where(rng.integers(0, 2, len(oo)) == 0, np.inf, 2.5)))
                for length in (1e30, 1e38):
                    huge.append(rays8(oo, (sgn * nrm[keep] + 0.2 * _sphere(rng, len(oo))) * length, tm[keep], np.inf if sgn < 0 else float(FMAX)))
        self.add("D", np.concatenate(rays))
        self.add("D2", np.concatenate(huge))
        m = 1500
        tm = _times(rng, m)
        a, b = _inside(rng, m, 0.95), _inside(rng, m, 0.95)
        on = rng.integers(0, g.n, m)
        for r in range(g.n):      # half of them start on a rectangle, as a path vertex does
            sel = (on == r) & (np.arange(m) % 2 == 0)
            a[sel] = g.point(r, rng.uniform(-.95, .95, sel.sum()), rng.uniform(-.95, .95, sel.sum()), tm[sel])
        a, b = a.astype(F32), b.astype(F32)
        dv = (b - a).astype(F32)
        dist = np.sqrt((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]).astype(F32) + dv[:, 2] * dv[:, 2]).astype(F32)
        self.add("S", rays8(a, dv / dist[:, None], tm, dist * (F32(1) - SHADOW_EPS)))

    # ---- E
    def _parallel(self, rng):
        g, rays = self.geo, []
        denorm = [1.4e-45, 4.2e-45, 1.1e-44, 1e-42, 1e-39]
        for r in range(g.n):
            eu, ev, n = g.axes(r)
            # origins: off the plane, and the origins family D found in (or next to) the plane of this rectangle
            oo, tt, ss = self.plane_origins[2]
            in_plane = oo[ss == r][:6]
            origins = np.concatenate([_inside(rng, 6), in_plane]) if len(in_plane) else _inside(rng, 6)
            tm = np.concatenate([_times(rng, 6), tt[ss == r][:6]]) if len(in_plane) else _times(rng, 6)
            m = len(origins)
            for s in denorm:
                for maxt in (np.inf, 5.0):
                    rays.append(rays8(origins, (_sphere(rng, m) * s), tm, maxt))
            # directions in the plane, their component along the normal's main axis bisected to the sign change of the local z
            ax = int(np.argmax(np.abs(n)))
            ang = rng.uniform(0, 2 * np.pi, m)
            d = (np.cos(ang)[:, None] * eu / np.linalg.norm(eu) + np.sin(ang)[:, None] * ev / np.linalg.norm(ev)).astype(F32)
            o32 = origins.astype(F32)

            def zy(x, keep):
                dd = d[keep].copy()
                dd[:, ax] = x
                return self.oracle(rays8(o32[keep], dd, tm[keep], np.inf))["ops"][:, r, ZY]
            xa, xb = (d[:, ax] - F32(0.01)).astype(F32), (d[:, ax] + F32(0.01)).astype(F32)
            za, zb = zy(xa, slice(None)), zy(xb, slice(None))
            keep = np.sign(za) * np.sign(zb) < 0
            if keep.any():
                sa = np.sign(za[keep])
                lo, hi = bisect(lambda x: zy(x, keep) * sa > 0, xa[keep], xb[keep])
                toward = np.sign(ordf(hi) - ordf(lo))
                for k in (-1, 0, 1, 2):
                    dd = d[keep].copy()
                    dd[:, ax] = unordf(ordf(lo) + toward * k)
                    for maxt in (np.inf, 5.0):
                        rays.append(rays8(o32[keep], dd, tm[keep], maxt))
        self.add("E", np.concatenate(rays))

    # ---- F
    def _ties(self, rng, m=400):
        g, rays = self.geo, []
        for r in range(g.n):
            tm = _times(rng, m)
            tm[::2] = 0.0      # the wall is in its start pose at time 0
            q = g.point(r, rng.uniform(-1.1, 1.1, m), rng.uniform(-1.1, 1.1, m), tm)
            o = _inside(rng, m, 1.2)
            rays.append(rays8(o, q - o, tm, np.where(rng.integers(0, 2, m) == 0, np.inf, 3.0)))
        self.add("F", np.concatenate(rays))

    # ---- G
    def _wall(self, rng, m=400):
        g, rays = self.geo, []
        for r in g.instances:
            ta, tb = _times(rng, m), _times(rng, m)
            ta[::4], tb[::4] = 0.0, SHUTTER
            q = g.point(r, rng.uniform(-1.2, 1.2, m), rng.uniform(-1.2, 1.2, m), ta)
            o = np.stack([rng.uniform(-.9, .9, m), rng.uniform(.1, 1.9, m), rng.uniform(-.5, 1.5, m)], 1)
            first, second = rays8(o, q - o, ta, np.inf), rays8(o, q - o, tb, np.inf)
            rays += [first, second]
            t1, t2 = self.oracle(first)["ops"][:, r, T], self.oracle(second)["ops"][:, r, T]
            mid = ((t1.astype(np.float64) + t2) / 2).astype(F32)
            both = np.isfinite(mid) & (t1 != t2)
            for x in (first, second):
                y = x[both].copy()
                y[:, 7] = mid[both]
                rays.append(y)
        if rays:
            self.add("G", np.concatenate(rays))

    # ---- H, HT, X
    def _extreme(self, rng):
        a = self.of("A")
        res = self.oracle(a, False)
        base = a[res["obj"] >= 0][:6].copy()
        base[:, 7] = np.inf
        bad = []
        for col in range(6):
            for val in (np.nan, np.inf, -np.inf):
                x = base.copy(); x[:, col] = val; bad.append(x)
        for val in (np.nan, -np.inf):
            x = base.copy(); x[:, 7] = val; bad.append(x)
        for z in (0.0, -0.0):
            x = base.copy(); x[:, 3:6] = z; bad.append(x)
        for col in (0, 1, 2, None):
            for length in (1.0, 1e-30, 1e30):
                x = base.copy()
                x[:, 0:3] = 1e30 if col is None else x[:, 0:3]
                if col is not None:
                    x[:, col] = 1e30 * (1 if length == 1.0 else -1)
                x[:, 3:6] = (x[:, 3:6].astype(np.float64) * length).astype(F32)
                bad.append(x)
        self.add("H", np.concatenate(bad))
        ht = []
        for val in (np.nan, np.inf, -np.inf):
            x = base.copy(); x[:, 6] = val; ht.append(x)
        self.add("HT", np.concatenate(ht))
        x = a[:400].copy()
        with np.errstate(over="ignore"):
            scale = np.array([1e-30, 1e30, 1e38, 1e-38, 1e-42])[np.arange(len(x)) % 5]
            x[:, 3:6] = (x[:, 3:6].astype(np.float64) * scale[:, None]).astype(F32)
        self.add("X", x)

    # ---- M
    def _misses(self, rng, m=256):
        o = np.stack([rng.uniform(-.2, .2, m), rng.uniform(.8, 1.2, m), rng.uniform(40, 60, m)], 1)
        d = np.stack([rng.uniform(-.2, .2, m), rng.uniform(-.2, .2, m), np.ones(m)], 1)
        d[np.abs(d[:, 0]) < 0.02, 0] = 0.05      # (a direction in a wall's plane has no certain answer)
        d[np.abs(d[:, 1]) < 0.02, 1] = -0.05
        self.add("M", rays8(o, d, _times(rng, m), 1.0))

    # ---- C, C2
    def _maxt(self, rng, per_rect=1200):
        src = self.of("A", "A2", "B", "D", "D2", "S", "E", "F", "G", "X")
        src = src[np.isfinite(src).all(axis=1) | (np.isfinite(src[:, :7]).all(axis=1) & (src[:, 7] == np.inf))]
        ops = self.oracle(src)["ops"]
        ok = passes(ops)
        out = []
        for r in range(self.geo.n):
            rows = np.flatnonzero(ok[:, r])
            if len(rows) > per_rect:      # keep the rarest first: rays that start in the plane (t == 0), then a random choice of the rest
                zero = rows[ops[rows, r, T] == 0]
                rest = np.setdiff1d(rows, zero)
                rows = np.concatenate([zero[:per_rect // 4], rng.choice(rest, per_rect - min(len(zero), per_rect // 4), replace=False)])
            t = ops[rows, r, T]
            for k in (-1, 0, 1):
                y = src[rows].copy()
                y[:, 7] = step(t, k)
                out.append(y)
            # ... and either side of the certain-miss test's own bound, flat_cull_far(maxt) = maxt (1 + 2^-20): a maxt so far below t that the z row settles the
            # rectangle, and one between, where the full test has to find t > maxt
            for factor in (1 - 2.0 ** -19, 1 - 2.0 ** -21):
                y = src[rows[::4]].copy()
                y[:, 7] = (t[::4] * F32(factor)).astype(F32)
                out.append(y)
        self.add("C", np.concatenate(out))
        base = np.concatenate([self.of("D")[::3], self.of("D2")[::3], self.of("A")[:200]])
        special = []
        for val in (0.0, -0.0, 1.4e-45, 2.0 ** -100, -1.0):
            y = base.copy(); y[:, 7] = val; special.append(y)
        self.add("C2", np.concatenate(special))

    # ---- the third placement
    def _short_lists(self):
        """{label: (indices into self.rays)} lists of 1, 63, 64, 65 rays: certain misses (M) around ONE ray that hits, and a list of certain misses only"""
        miss = np.flatnonzero(self.family == "M")
        hits = np.flatnonzero((self.family == "A") & (self.want["obj"] >= 0) & (self.want["occluded"] == 1))
        per_obj = [hits[self.want["obj"][hits] == o][:1] for o in np.unique(self.want["obj"][hits])]
        hit = np.concatenate(per_obj)
        self.short = {}
        for k, h in enumerate(hit):
            for n, at in ((1, 0), (63, 17), (64, 40), (64, 0), (64, 63), (65, 64), (65, 5)):
                rows = miss[(np.arange(n) + 7 * k) % len(miss)].copy()
                rows[at] = h
                self.short["hit %d: %d rays, the hit in lane %d" % (k, n, at)] = rows
        # ... and ONE ray ON a bound among certain misses: a wave runs a rectangle's full test when any of its lanes needs it, for all of its lanes, so a lane the
        # certain-miss test settles wrongly still gets the right answer beside a neighbour that needs the test.  Alone among certain misses it does not.  Rays of C
        # with t == maxt that hit nothing else (occluded, no closest hit), the exact quotient -zx / zy above maxt (t was rounded DOWN onto it: the case flat_cull_far
        # has to stay strictly above maxt for) and below it; and rays that start in a rectangle's plane (t = +-0).
        c = np.flatnonzero((self.family == "C") & self.finite)
        ops, maxt = self.want["ops"][c], self.rays[c, 7]
        ok = passes(ops, maxt)
        with np.errstate(all="ignore"):
            exact = -ops[..., ZX].astype(np.float64) / ops[..., ZY].astype(np.float64)
        for r in range(self.geo.n):
            alone = ok[:, r] & (ok.sum(axis=1) == 1) & (self.want["occluded"][c] == 1)
            at = alone & (ops[:, r, T] == maxt) & (maxt > 0)
            picks = [("t == maxt rounded down", c[at & (exact[:, r] > maxt)][:2]), ("t == maxt rounded up", c[at & (exact[:, r] < maxt)][:1]),
                     ("t == 0", c[alone & (ops[:, r, T] == 0)][:1])]
            for what, rows_ in picks:
                for j, h in enumerate(rows_):
                    for n, at_lane in ((1, 0), (64, 21), (65, 64)):
                        rows = miss[(np.arange(n) + 11 * r + j) % len(miss)].copy()
                        rows[at_lane] = h
                        self.short["rectangle %d, %s (%d): %d rays, that ray in lane %d" % (r, what, j, n, at_lane)] = rows
        self.only_misses = miss[:128]


# ---------------------------------------------------------------------------- the device side
def device_query(mi, scene, form, any_hit, rays):
    """dtof_flat_query into buffers pre-filled with CANARY -> (return code, (n, 3) t, u, v as uint32 or None, (n,) ids as int32)"""
    rays = np.ascontiguousarray(rays, F32).reshape(-1, 8)
    out, ids = np.full((len(rays), 3), CANARY, np.uint32), np.full(len(rays), CANARY, np.uint32)
    rc = mi._lib().dtof_flat_query(scene._h, form, 1 if any_hit else 0, len(rays), rays.ctypes.data, None if any_hit else out.ctypes.data, ids.ctypes.data)
    return rc, (None if any_hit else out), ids.view(np.int32)


def want_words(sweep, any_hit, rows=slice(None)):
    """the oracle's answer in the words dtof_flat_query writes: ((n, 3) uint32 or None, (n,) int32)"""
    w = sweep.want
    if any_hit:
        return None, w["occluded"][rows].astype(np.int32)
    return np.stack([w["t"][rows], w["u"][rows], w["v"][rows]], 1).view(np.uint32), w["obj"][rows].astype(np.int32)


def describe(sweep, rows, got, want, what, limit=6):
    """the first few rays that differ: family, ray, both answers and the oracle's operands of every rectangle"""
    fam, cnt = np.unique(sweep.family[rows], return_counts=True)
    lines = ["%s: %d of %d rays differ; by family: %s" % (what, len(rows), sweep.n, ", ".join("%s %d" % (f, c) for f, c in zip(fam, cnt)))]
    for i in rows[:limit]:
        lines.append("  ray %d, family %s: o %s d %s time %r maxt %r" % (i, sweep.family[i], sweep.rays[i, 0:3].tolist(), sweep.rays[i, 3:6].tolist(), float(sweep.rays[i, 6]), float(sweep.rays[i, 7])))
        lines.append("    device %s   oracle %s" % (got(i), want(i)))
        for r in range(sweep.geo.n):
            zx, zy, t, u, v, best = (float(x) for x in sweep.want["ops"][i, r])
            lines.append("    rectangle %d (object %d): zx %r zy %r t %r u %r v %r best %r" % (r, sweep.want["rect_obj"][r], zx, zy, t, u, v, best))
    return "\n".join(lines)


# ---------------------------------------------------------------------------- the compares, classified from the oracle's operands
def compare_classes(sweep):
    """{(rectangle, compare): (below, on, above)} over the finite rays, each compare counted only where the rectangle's other compares pass (so that it decides);
    `t < best` among the rays that pass all four"""
    ops, maxt = sweep.want["ops"][sweep.finite], sweep.rays[sweep.finite, 7]
    out = {}
    with np.errstate(invalid="ignore"):
        for r in range(sweep.geo.n):
            t, u, v, best = ops[:, r, T], np.abs(ops[:, r, U]), np.abs(ops[:, r, V]), ops[:, r, BEST]
            c = {"t >= 0": (t, np.zeros_like(t), (t <= maxt) & (u <= 1) & (v <= 1)), "t <= maxt": (t, maxt, (t >= 0) & (u <= 1) & (v <= 1)),
                 "|u| <= 1": (u, np.ones_like(u), (t >= 0) & (t <= maxt) & (v <= 1)), "|v| <= 1": (v, np.ones_like(v), (t >= 0) & (t <= maxt) & (u <= 1)),
                 "t < best": (t, best, (t >= 0) & (t <= maxt) & (u <= 1) & (v <= 1))}
            for name, (a, b, others) in c.items():
                out[(r, name)] = (int((others & (a < b)).sum()), int((others & (a == b)).sum()), int((others & (a > b)).sum()))
    return out


CULL_SOURCE = """#include "dtof_flat_cull.h"
extern "C" void flat_sweep_cull(unsigned n, const float *zx, const float *zy, const float *maxt, unsigned char *out) {
    for (unsigned i = 0; i < n; ++i) out[i] = dtof::flat_certain_miss(zx[i], zy[i], dtof::flat_cull_far(maxt[i])) ? 1 : 0;
}
"""


def host_cull(lib, zx, zy, maxt):
    """flat_certain_miss(zx, zy, flat_cull_far(maxt)) of the HOST compilation of dtof_flat_cull.h, elementwise"""
    zx, zy, maxt = (np.ascontiguousarray(np.broadcast_to(a, np.broadcast(zx, zy, maxt).shape), F32).ravel() for a in (zx, zy, maxt))
    out = np.zeros(len(zx), np.uint8)
    lib.flat_sweep_cull(C.c_uint(len(zx)), zx.ctypes.data_as(C.c_void_p), zy.ctypes.data_as(C.c_void_p), maxt.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out.astype(bool)

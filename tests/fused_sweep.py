"""Scenes and ray families of the fused sweep (test_fused_sweep_cpu.py, test_fused_sweep_gpu.py): the tree walk the fused shade kernels run themselves -- trace_scene with
the instance memo, the resident stage's SOA node planes, the 16-bit child references and stack columns, the block-size stack stride, through dtof_fused_query -- and the
analytic shapes' ray tests (sphere_hit<ANY>, cylinder_hit, disk_hit of mitsuba3dopplertof_amd/csrc/dtof_traverse.h) on rays placed ON their decisions, against the
oracle's brute-force scene_closest / scene_occluded over the same rays (orc_kat_tree_n).

Scenes, written into a directory from scenes/make_scenes.py pieces (`forms` = (form, waves) of dtof_fused_query a scene meets on a device with 160 KiB of LDS per block;
every scene also meets form 0 of dtof_tree_query):

  analytic_field  44 static spheres, disks and cylinders -- plain, with flip_normals, under rotated and uniformly scaled to_world, three with exact float centre / pole /
                  axis, one of each at coordinates around 100 -- nine rectangles and ONE moving instance of a group of a 12-triangle cube, a sphere, a disk and a
                  cylinder.  Ties at equal float t: two equal spheres as two objects, a disk touching a sphere's pole, a disk coplanar with a rectangle in both object
                  orders (axis-aligned, and a small disk over a larger rectangle in a tilted plane, where the rectangle's box is entered first), a static sphere
                  where the group's sphere is at time 0.  Blob above 16 KiB, record block within 24 KiB: forms 0 (global blob), 2, 3 WITH a memo object.
  analytic_small  one of each shape, the ties and the instance within 16 KiB: form 0 with the blob staged in LDS.
  rects_tree      twelve rectangles and one moving instance of a rectangle: forms 0 and 1.
  domino_field    make_scenes.domino(n_side=14): 196 moving instances of one cube, no memo object: forms 0, 2, 3.
  domino_half     make_scenes.domino(n_side=33): 1 089 instances, a TLAS of 1 025 .. 2 048 nodes: forms 0, 4, 5.  A few thousand rays: the oracle is brute force.

Ray families (the label of a ray; every ray serves both query kinds; directions are normalised in float32, origins lie within 1e4 extents).  Every threshold is bisected ON
THE ORACLE, on the hit or miss of the ONE shape (tree_n(per_prim=True)), to the last float that still hits, and issued three floats either side.  The sphere's occlusion
form is another quadratic: its thresholds are bisected again on the occlusion flag of a scene that holds that sphere alone.

  S   sphere: tangent rays from 1, 10, 1e2, 1e4 radii, oblique and axis-aligned; origins inside (the far root) and on the surface; maxt bisected around near_t from outside
      and around far_t from inside (in_bounds), and a float either side of far_t from outside; the sphere just behind the origin (far_t around 0); origins with
      l . d == 0 exactly, with and without a coordinate equal to the centre's, inside and outside; the origin at the centre.
  Y   cylinder: tangent to the wall; hits bisected across both ends (z == 0, z == 1); through an open end onto the wall from inside (!near_ok && far_ok), bisected across
      the far end; parallel to the axis inside, on and outside the wall (A == 0; on the exact cylinder the local direction is exactly axial); maxt bisected around the
      near root from outside and the far root from the axis; the flipped, the scaled and the instanced cylinder.
  K   disk: the rim bisected along eight azimuths; the centre; rays in the plane (ld.z == +0, -0; origin in and off the plane); t bisected around 0 and around maxt.
  T   ties as built into the scene, from 1, 10 and 100 away.
  G   the moving group's analytic shapes (Domino: the cubes) at both shutter ends and between, maxt inf and between the two distances.
  A   random: origins around a shape, half of the directions uniform and half towards a point of a shape; times over the shutter; maxt inf / FLT_MAX / finite.
  M   certain misses: origins far outside that fly away, finite maxt.
  C   every hit of the families above with maxt the float below t, t itself (a miss) and the float above.
  H   non-finite and extreme rays (NaN, +-inf in every component in turn, maxt NaN / -inf, zero directions, origins at 1e30, directions of length 1e-30 .. 1e38, times
      NaN / +-inf -- also on G's rays that reach the instance at one shutter end only), sent only where the oracle misses.

Placements: the families in order, one fixed permutation, and the one hit among certain misses in lists of 1, 63, 64, 65 rays and, for the resident forms, of
waves * 64 - 1, waves * 64 and waves * 64 + 1.  Everything is a function of SEED."""
import os
import sys

import numpy as np

import tree_sweep as ts
from conftest import SCENES

sys.path.insert(0, SCENES)
import make_scenes as ms      # noqa: E402

F32 = np.float32
SEED = 20261021
SHUTTER = ts.SHUTTER
FMAX = ts.FMAX
CANARY = ts.CANARY
KINDS = ts.KINDS
FORM_NAMES = ("classic", "classic_rect", "resident", "resident_16", "resident_half", "resident_half_16")
WAVES = (8, 12, 16)
LDS_LIMIT = 160 * 1024 - 1024      # device_lds_limit() on gfx950: 160 KiB per block less k_shade's static LDS
RECT, MESH, SPHERE, DISK, CYLINDER = 0, 1, 2, 3, 4
KIND_NAMES = {RECT: "rect", MESH: "mesh", SPHERE: "sphere", DISK: "disk", CYLINDER: "cylinder"}
# (form, waves) a scene meets; waves = 0 for the classic forms.  analytic_field carries a memo column per wave: at 16 waves the 32-bit stack columns no longer fit
SCENE_FORMS = [
    ("analytic_field", ((0, 0), (2, 8), (2, 12), (3, 8), (3, 12), (3, 16))),
    ("analytic_small", ((0, 0),)),
    ("rects_tree", ((0, 0), (1, 0))),
    ("domino_field", ((0, 0), (2, 8), (2, 12), (2, 16), (3, 8), (3, 12), (3, 16))),
    ("domino_half", ((0, 0), (4, 8), (4, 12), (4, 16), (5, 8), (5, 12), (5, 16))),
]
NAMES = [n for n, _ in SCENE_FORMS]
CASES = [(n, f, w, k) for n, forms in SCENE_FORMS for f, w in forms for k in KINDS]
TREE_FORM_0 = ("analytic_field", "analytic_small")      # ... whose new families also go through dtof_tree_query form 0


def case_id(n, f, w, k):
    return "%s-%s%s-%s" % (n, FORM_NAMES[f], "-%dw" % w if w else "", k)


# ---------------------------------------------------------------------------- scenes
def _tw(*ops):
    return '<transform name="to_world">' + "".join(ops) + "</transform>"


def _sc(v):
    return '<scale value="%s"/>' % v


def _rot(axis, angle):
    return '<rotate %s="1" angle="%s"/>' % (axis, angle)


def _tr(x, y, z):
    return '<translate x="%s" y="%s" z="%s"/>' % (x, y, z)


def _shape(kind, body, ident=None, bsdf="TallBoxBSDF", flip=False):
    return ('<shape type="%s"%s>%s%s<ref id="%s"/></shape>\n'
            % (kind, ' id="%s"' % ident if ident else "", body, '<boolean name="flip_normals" value="true"/>' if flip else "", bsdf))


def _sphere(c, r, ident=None, flip=False, xf=""):
    return _shape("sphere", '<point name="center" x="%s" y="%s" z="%s"/><float name="radius" value="%s"/>%s' % (c[0], c[1], c[2], r, xf), ident, flip=flip)


def _cyl(p0, p1, r, ident=None, flip=False):
    return _shape("cylinder", '<point name="p0" x="%s" y="%s" z="%s"/><point name="p1" x="%s" y="%s" z="%s"/><float name="radius" value="%s"/>' % (tuple(p0) + tuple(p1) + (r,)),
                  ident, "ShortBoxBSDF", flip)


# The named static spheres, ONE definition each: the scenes and the one-sphere scenes on which the occlusion thresholds are bisected (solo) are built from it
BALLS = {"ExactBall": ((0, 1, 0), 0.5, False, ""),      # pole (0, 1.5, 0)
         "PlainBall": ((-1.3, 0.4, 0.7), 0.3, False, ""), "FlipBall": ((1.1, 0.45, 1.6), 0.35, True, ""),
         "TurnedBall": ((0.2, 0.1, -0.3), 0.4, False, _tw(_sc("1.5"), _rot("y", "35"), _rot("x", "-20"), _tr("-3", "2.5", "-2"))),
         "FarBall": ((100.25, 99.5, 101), 2, False, "")}
SOLO_BALLS = ("ExactBall", "FlipBall", "TurnedBall", "FarBall")


def _ball(ident):
    c, r, flip, xf = BALLS[ident]
    return _sphere(c, r, ident, flip=flip, xf=xf)


GROUP = ('<shape type="shapegroup" id="G">'
         '<shape type="cube">' + _tw(_sc("0.25"), _tr("0", "0.25", "1")) + '<ref id="ShortBoxBSDF"/></shape>\n' +
         _sphere((0, 1, 0), 0.5) + _shape("disk", _tw(_sc("0.5"), _rot("x", "-90"), _tr("1.5", "0.5", "0"))) + _cyl((-1.5, 0, 0), (-1.5, 1, 0), 0.25) +
         '</shape>\n')
# the ONE instance: at time 0 a translation by exact floats, so that the static sphere OutsideTwin lies where the group's sphere does
INSTANCE = ('<shape type="instance"><ref id="G"/><animation name="to_world"><transform time="0"><translate x="8" y="0" z="0"/></transform>'
            '<transform time="%s"><translate x="8" y="0" z="0.25"/></transform></animation></shape>\n' % SHUTTER)
# the ties and one exact shape of each kind (centre, pole and axis are exact floats); rays for them: TIE_RAYS
CORE = (_ball("ExactBall") +
        _shape("disk", _tw(_sc("0.5"), _rot("x", "-90"), _tr("0", "1.5", "0")), "PoleDisk") +                           # ... which this disk touches, normal +y
        _sphere((2, 1, -1), 0.25, "TwinA") + _sphere((2, 1, -1), 0.25, "TwinB") +
        _shape("disk", _tw(_sc("0.5"), _tr("-2", "1", "0")), "DiskOverRect") + _shape("rectangle", _tw(_sc("0.75"), _tr("-2", "1", "0")), "RectUnderDisk") +
        _shape("rectangle", _tw(_sc("0.75"), _tr("-4", "1", "0")), "RectOverDisk") + _shape("disk", _tw(_sc("0.5"), _tr("-4", "1", "0")), "DiskUnderRect") +
        _shape("cylinder", _tw(_sc("0.5"), _tr("3", "0.5", "-1")), "ExactPipe", "ShortBoxBSDF") +                        # axis along z from (3, 0.5, -1), radius and length 0.5
        _shape("disk", _tw(_sc("0.5"), _tr("4.5", "1", "-2")), "ExactDisk") +                                          # in the plane z = -2
        _sphere((8, 1, 0), 0.5, "OutsideTwin") +
        # ... and the coplanar pairs again with the DISK the larger of the two (the thicker padded box: the walk meets it first), in both object orders
        _shape("disk", _tw(_sc("1"), _tr("-6", "1", "0")), "WideDiskOverRect") + _shape("rectangle", _tw(_sc("0.5"), _tr("-6", "1", "0")), "RectUnderWideDisk") +
        _shape("rectangle", _tw(_sc("0.5"), _tr("-9", "1", "0")), "RectOverWideDisk") + _shape("disk", _tw(_sc("1"), _tr("-9", "1", "0")), "WideDiskUnderRect") +
        # ... and in a TILTED plane, the disk first and the smaller: the padded boxes of an axis-aligned plane are equally thick and the walk takes the left child first,
        # here the rectangle's box is entered before the disk's, so the disk comes second with the lower index and only the tie clause gives it the hit
        _shape("disk", _tw(_sc("0.25"), _rot("x", "30"), _tr("-12", "1", "0")), "SmallDiskOverTiltedRect") +
        _shape("rectangle", _tw(_sc("1"), _rot("x", "30"), _tr("-12", "1", "0")), "TiltedRectUnderDisk"))
TIE_RAYS = [((0, 3, 0), (0, -1, 0)), ((2, 3, -1), (0, -1, 0)), ((2, 1, 2), (0, 0, -1)), ((-2, 1, 2), (0, 0, -1)), ((-2.25, 1.125, 3), (0, 0, -1)),
            ((-4, 1, 2), (0, 0, -1)), ((-4.25, 0.875, -3), (0, 0, 1)), ((8, 3, 0), (0, -1, 0)), ((8, 1, 2), (0, 0, -1)), ((8.25, 1, -3), (0, 0, 1)),
            ((-2, 1, -2), (0, 0, 1)), ((-2.25, 0.875, -3), (0, 0, 1)), ((-4.125, 1.25, 2), (0, 0, -1)),
            ((-6, 1, 2), (0, 0, -1)), ((-6.25, 1.125, -3), (0, 0, 1)), ((-5.75, 0.75, 4), (0, 0, -1)), ((-9, 1, 2), (0, 0, -1)), ((-9.25, 0.875, -3), (0, 0, 1)),
            ((-8.75, 1.25, 4), (0, 0, -1))]
TILT_N = np.array([0.0, -np.sin(np.pi / 6), np.cos(np.pi / 6)])      # the tilted pair's normal: rays along it, both ways, through the small disk
TIE_RAYS += [(tuple(np.array([-12.0 + dx, 1.0, 0.0]) + s * 2.0 * TILT_N), tuple(-s * TILT_N)) for dx in (0.0, 0.125, -0.0625) for s in (1.0, -1.0)]


def _field_extras(rng):
    """the rest of analytic_field: flipped, rotated, scaled and far shapes, then random ones up to 44 analytic shapes, and four rectangles"""
    s = (_ball("PlainBall") + _ball("FlipBall") + _ball("TurnedBall") + _ball("FarBall") +
         _shape("disk", _tw(_sc("0.3"), _rot("x", "-70"), _tr("0.6", "1.2", "-0.5")), "TiltDisk") +
         _shape("disk", _tw(_sc("0.4"), _rot("y", "50"), _tr("1.5", "2.2", "0.8")), "FlipDisk", flip=True) +
         _shape("disk", _tw(_sc("3"), _rot("z", "25"), _rot("x", "40"), _tr("104", "97", "99")), "FarDisk") +
         _cyl((-0.8, 0.2, 0.6), (-0.6, 1.0, 0.7), 0.12, "PlainPipe") + _cyl((0.4, 0.1, 2.2), (0.9, 0.2, 2.6), 0.2, "FlipPipe", flip=True) +
         _shape("cylinder", _tw(_sc("0.3"), _rot("x", "-70"), _rot("z", "15"), _tr("2.6", "2.2", "0.4")), "TurnedPipe", "ShortBoxBSDF") +
         _cyl((96, 101, 100), (99, 103, 98), 1.5, "FarPipe"))
    n = 17 + 11      # CORE has 12 analytic shapes + 5 rectangles, the lines above 11
    k = 0
    while n - 5 < 44:
        c = np.round(rng.uniform((12, 0.2, -4), (24, 3.5, 4)), 3)      # (beside the ties, not across their rays)
        r = round(float(rng.uniform(0.08, 0.3)), 3)
        if k % 3 == 0:
            s += _sphere(c, r, "Ball%d" % k, flip=k % 2 == 1)
        elif k % 3 == 1:
            s += _shape("disk", _tw(_sc(r), _rot("xyz"[k % 3], round(float(rng.uniform(-90, 90)), 1)), _rot("y", round(float(rng.uniform(0, 180)), 1)), _tr(*c)), "Disk%d" % k, flip=k % 2 == 1)
        else:
            s += _cyl(c, np.round(c + rng.uniform(-0.5, 0.5, 3), 3), r, "Pipe%d" % k, flip=k % 2 == 1)
        n, k = n + 1, k + 1
    for k in range(4):
        s += _shape("rectangle", _tw(_sc(round(float(rng.uniform(0.2, 0.6)), 3)), _rot("x", round(float(rng.uniform(-90, 90)), 1)), _tr(*np.round(rng.uniform((12, 0.2, -4), (24, 3.5, 4)), 3))), "Card%d" % k)
    return s


def _rects(rng):
    s = ""
    for name, m, b in ms.WALLS:
        s += ms.rect(name, m, b)
    for k in range(7):
        s += _shape("rectangle", _tw(_sc(round(float(rng.uniform(0.15, 0.5)), 3)), _rot("xyz"[k % 3], round(float(rng.uniform(-80, 80)), 1)), _tr(*np.round(rng.uniform((-0.8, 0.2, -0.8), (0.8, 1.8, 0.8)), 3))), "Card%d" % k)
    s += ('<shape type="shapegroup" id="G"><shape type="rectangle">' + _tw(_sc("0.3"), _rot("y", "30")) + '<ref id="ShortBoxBSDF"/></shape></shape>\n'
          '<shape type="instance"><ref id="G"/><animation name="to_world"><transform time="0"><translate x="0.2" y="1" z="0.1"/></transform>'
          '<transform time="%s"><translate x="0.2" y="1" z="0.3"/></transform></animation></shape>\n' % SHUTTER)
    return s


def build(name, d):
    """writes the scene `name` into the directory d -> path of the XML file"""
    rng = np.random.default_rng([SEED, 7, NAMES.index(name)])
    if name == "analytic_field":
        s = ts._head() + CORE + _field_extras(rng) + GROUP + INSTANCE + ms.LIGHT + "</scene>\n"
    elif name == "analytic_small":
        s = ts._head() + CORE + GROUP + INSTANCE + ms.LIGHT + "</scene>\n"
    elif name == "rects_tree":
        s = ts._head() + _rects(rng) + ms.LIGHT + "</scene>\n"
    elif name in ("domino_field", "domino_half"):
        s = ms.domino(n_side=14 if name == "domino_field" else 33, res=16, spp=4)
    else:
        raise KeyError(name)
    path = os.path.join(str(d), name + ".xml")
    open(path, "w").write(s)
    return path


def solo(ident, d):
    """a scene that holds the sphere BALLS[ident] alone (the sphere's occlusion thresholds are bisected on its occlusion flag)"""
    path = os.path.join(str(d), "solo_%s.xml" % ident)
    open(path, "w").write(ts._head() + _ball(ident) + ms.LIGHT + "</scene>\n")
    return path


# ---------------------------------------------------------------------------- the primitives of a scene
class Prim:
    """one non-mesh shape: its object, its shape index in the group, its per_prim slot and its frame -- world point = O + x U + y V + z W of the unit shape (sphere of
    radius 1 at 0; disk of radius 1 and rectangle [-1, 1]^2 in z = 0; cylinder of radius 1 around z, 0 <= z <= 1) -- in the object's space; `ob`: the instance or None"""

    def __init__(self, obj, shape, slot, sh, ob):
        self.obj, self.shape, self.slot, self.kind, self.ob = obj, shape, slot, sh["kind"], ob
        m = np.asarray(sh["to_world"], np.float64).reshape(4, 4)
        lin, off = m[:3, :3], m[:3, 3]
        if self.kind == SPHERE:      # (orc.Scene has composed centre and radius with to_world: sphere_baked = world centre, world radius)
            self.O = np.asarray(sh["sphere_baked"][:3], np.float64)
            self.U, self.V, self.W = float(sh["sphere_baked"][3]) * np.eye(3)
        else:      # (... and the cylinder's p0, p1 and radius: to_world maps the unit cylinder)
            self.O, self.U, self.V, self.W = off, lin[:, 0], lin[:, 1], lin[:, 2]
        self.size = float(max(np.linalg.norm(self.U), np.linalg.norm(self.W) if self.kind == CYLINDER else 0.0))

    def moving(self):
        return self.ob is not None and self.ob["n_keys"] > 1

    def frame(self, time=0.0):
        k = ts.Geometry.matrix(self.ob, time)
        return k[:3, :3] @ self.O + k[:3, 3], k[:3, :3] @ self.U, k[:3, :3] @ self.V, k[:3, :3] @ self.W

    def at(self, xyz, time=0.0):
        o, u, v, w = self.frame(time)
        xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
        return o + xyz[:, 0:1] * u + xyz[:, 1:2] * v + xyz[:, 2:3] * w

    def surface(self, rng, n):
        """n points of the unit shape"""
        if self.kind == SPHERE:
            return ts._sphere(rng, n)
        th = rng.uniform(0, 2 * np.pi, n)
        if self.kind == CYLINDER:
            return np.stack([np.cos(th), np.sin(th), rng.uniform(0, 1, n)], 1)
        if self.kind == DISK:
            rho = np.sqrt(rng.uniform(0, 1, n))
            return np.stack([rho * np.cos(th), rho * np.sin(th), np.zeros(n)], 1)
        return np.concatenate([rng.uniform(-1, 1, (n, 2)), np.zeros((n, 1))], 1)

    def bounds(self, time=0.0):
        """float64 world bounds at `time`"""
        o, u, v, w = self.frame(time)
        if self.kind == SPHERE:
            r = np.linalg.norm(u)
            return o - r, o + r
        if self.kind == RECT:
            e = np.abs(u) + np.abs(v)
            return o - e, o + e
        e = np.sqrt(u * u + v * v)
        if self.kind == DISK:
            return o - e, o + e
        return np.minimum(o, o + w) - e, np.maximum(o, o + w) + e


class MeshPrim:
    """a triangle mesh of ts.Geometry in the same clothes"""

    def __init__(self, geo, m):
        self.geo, self.m, self.obj, self.shape, self.kind, self.ob = geo, m, m["obj"], m["shape"], MESH, m["ob"]
        self.size = float(np.linalg.norm(geo.world(m, 0.0).max(0) - geo.world(m, 0.0).min(0)))

    def moving(self):
        return self.ob is not None and self.ob["n_keys"] > 1

    def surface(self, rng, n):
        f = self.m["faces"][rng.integers(len(self.m["faces"]), size=n)]
        w = rng.dirichlet((1, 1, 1), n)
        return np.einsum("nk,nkc->nc", w, self.m["pos"][f])

    def at(self, pts, time=0.0):
        return self.geo.world(self.m, time, pts)

    def bounds(self, time=0.0):
        p = self.geo.world(self.m, time)
        return p.min(0), p.max(0)


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def norm32(d):
    """directions normalised in float32"""
    d = unit(d).astype(F32).reshape(-1, 3)
    return d / np.sqrt((d * d).sum(1, dtype=F32))[:, None].astype(F32)


def rays(o, d, time=0.0, maxt=np.inf):
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    n = max(len(o), len(d))
    r = np.zeros((n, 8), F32)
    r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7] = o, norm32(d), time, maxt
    return r


OBLIQUE, AXES = ts.OBLIQUE, ts.AXES


class Sweep:
    """the rays of one scene with their labels, placements and oracle answers"""

    def __init__(self, name, orc, directory):
        self.name, self.forms, self.dir = name, dict(SCENE_FORMS)[name], directory
        self.path = build(name, directory)
        self.orc = orc
        self.osc = orc.Scene(self.path, dict(resx=16, resy=16))
        self.small = name == "domino_half"
        self._prims()
        self.parts, self.bisected = [], {}
        rng = np.random.default_rng([SEED, NAMES.index(name)])
        self._random(rng, 800 if self.small else 5000 if name.startswith("domino") else 4000)
        if name.startswith("analytic"):
            self._spheres(rng)
            self._cylinders(rng)
            self._disks(rng)
            self._ties()
        self._instances(rng)
        self._misses(rng)
        self._maxt(rng)
        self._extreme(rng)
        self.rays = np.ascontiguousarray(np.concatenate([r for _, r, _ in self.parts]))
        self.family = np.concatenate([np.full(len(r), f, dtype="U2") for f, r, _ in self.parts])
        self.aim = np.concatenate([np.full(len(r), -1 if p is None else p, np.int64) for _, r, p in self.parts])      # index into self.prims of the shape a ray was built around
        self.n = len(self.rays)
        self.perm = np.random.default_rng([SEED, 99]).permutation(self.n)
        self.want = self.osc.tree_n(self.rays)
        self._short_lists()

    # ---- the scene's primitives, in the oracle's visit order
    def _prims(self):
        fs = self.osc.flat
        self.prims, slot = [], 0
        has_mesh = any(sh["kind"] == MESH for sh in fs.shapes)
        geo = ts.Geometry(self.osc) if has_mesh else None
        meshes = {(m["obj"], m["shape"]): m for m in geo.meshes} if geo else {}
        for oi, ob in enumerate(fs.objects):
            first, count = (ob["index"], 1) if ob["kind"] == 0 else (fs.groups[ob["index"]]["first_shape"], fs.groups[ob["index"]]["n_shapes"])
            for k in range(count):
                sh = fs.shapes[first + k]
                if sh["kind"] == MESH:
                    self.prims.append(MeshPrim(geo, meshes[(oi, k)]))
                    slot += len(meshes[(oi, k)]["faces"])
                else:
                    self.prims.append(Prim(oi, k, slot, sh, ob if ob["kind"] != 0 else None))
                    slot += 1
        self.by_id = {(p.obj, p.shape): i for i, p in enumerate(self.prims)}
        los, his = zip(*[p.bounds(t) for p in self.prims for t in (0.0, SHUTTER)])
        near = [i for i, (l, h) in enumerate(zip(los, his)) if np.abs(l).max() < 50 and np.abs(h).max() < 50]
        self.lo, self.hi = np.min([los[i] for i in near], 0), np.max([his[i] for i in near], 0)
        self.extent = float((self.hi - self.lo).max())

    def add(self, family, r, prim=None):
        if len(r):
            self.parts.append((family, np.ascontiguousarray(r, F32).reshape(-1, 8), prim))

    def of(self, *families):
        return np.concatenate([r for f, r, _ in self.parts if f in families])

    def analytic(self, kind):
        return [i for i, p in enumerate(self.prims) if p.kind == kind]

    # ---- bisection on the oracle
    def hits_prim(self, r, p):
        return ~np.isnan(self.osc.tree_n(r, per_prim=True)["prim_t"][:, p.slot])

    def bisect(self, hit, miss, col, test, label):
        """hit / miss: (m, 8) rays that differ in column `col` only -> the rays three floats either side of the last value of that column with which test(rays) is true;
        the pairs whose ends do not behave (hit misses or miss hits) are dropped and counted"""
        hit, miss = np.ascontiguousarray(hit, F32).reshape(-1, 8), np.ascontiguousarray(miss, F32).reshape(-1, 8)
        ok = test(hit) & ~test(miss)
        cnt = self.bisected.setdefault(label, [0, 0])
        cnt[0] += int(ok.sum()); cnt[1] += int((~ok).sum())
        hit, miss = hit[ok], miss[ok]
        if not len(hit):
            return np.zeros((0, 8), F32)
        lo, hi = ts.ordf(hit[:, col]), ts.ordf(miss[:, col])
        while (np.abs(hi - lo) > 1).any():
            mid = (lo + hi) // 2
            y = hit.copy(); y[:, col] = ts.unordf(mid)
            h = test(y)
            lo, hi = np.where(h, mid, lo), np.where(h, hi, mid)
        out = []
        for k in range(-3, 4):
            y = hit.copy(); y[:, col] = ts.unordf(lo - k * np.sign(hi - lo))
            out.append(y)
        return np.concatenate(out)

    @staticmethod
    def pair(base, col, a, b):
        """two copies of the rays `base` with column `col` set to a and to b"""
        h, m = np.array(base, F32).reshape(-1, 8), np.array(base, F32).reshape(-1, 8)
        h[:, col], m[:, col] = a, b
        return h, m

    # ---- A
    def _points(self, rng, n, times):
        idx = rng.integers(len(self.prims), size=n)
        pts = np.zeros((n, 3))
        for i in range(n):
            p = self.prims[idx[i]]
            pts[i] = p.at(p.surface(rng, 1), times[i])[0]
        return idx, pts

    def _random(self, rng, n):
        tm = ts._times(rng, n)
        idx, pts = self._points(rng, n, tm)
        size = np.array([self.prims[i].size for i in idx])
        o = pts + (1.0 + 5.0 * rng.uniform(size=(n, 1))) * size[:, None] * ts._sphere(rng, n)
        d = pts - o
        d[1::2] = ts._sphere(rng, len(d[1::2]))
        self.add("A", rays(o, d, tm, ts._maxts(rng, n, self.extent)))

    # ---- S
    def _spheres(self, rng):
        picks = [i for i in self.analytic(SPHERE)][:8] if self.name == "analytic_field" else self.analytic(SPHERE)
        for pi in picks:
            p = self.prims[pi]
            if p.moving():
                continue      # (family G)
            c, r = p.frame()[0], float(np.linalg.norm(p.frame()[1]))
            tests = [("closest", lambda y, p=p: self.hits_prim(y, p))]
            ident = self._ident(p)
            if ident in SOLO_BALLS and p.ob is None:
                alone = self.orc.Scene(solo(ident, self.dir), dict(resx=16, resy=16))
                mine, its = self._shape_record(p)["sphere_baked"], alone.flat.shapes[alone.flat.objects[0]["index"]]["sphere_baked"]
                assert np.array_equal(np.asarray(mine[:4]).view(np.uint32), np.asarray(its[:4]).view(np.uint32)), ident      # the same sphere, centre and radius bit for bit
                tests.append(("occlusion", lambda y, alone=alone: alone.tree_n(y)["occluded"] == 1))
            dirs = [unit(OBLIQUE[0]), unit(OBLIQUE[1]), AXES[0], AXES[3]]
            out = []
            for kind, test in tests:
                # tangents: the origin slides along a world axis, away from the line through the centre
                for dist in (1.0, 10.0, 1e2, 1e4):
                    for d in dirs:
                        k = int(np.argmin(np.abs(d)))
                        base = rays((c - (dist + 1.0) * r * d).astype(F32), d)
                        h, m = self.pair(base, k, base[0, k] + F32(0.5 * r), base[0, k] + F32(2.5 * r))
                        out.append(self.bisect(h, m, k, test, "S tangent, %s" % kind))
                # maxt: from outside around near_t, from inside around far_t (in_bounds)
                for d in dirs:
                    for start in (c - 3.0 * r * d, c + 0.3 * r * unit(OBLIQUE[2])):
                        h, m = self.pair(rays(start, d), 7, FMAX, 0.0)
                        out.append(self.bisect(h, m, 7, test, "S maxt, %s" % kind))
                # the sphere just behind the origin: far_t around 0
                for a in (0, 1, 2):
                    base = rays(c, AXES[2 * a])
                    h, m = self.pair(base, a, F32(c[a] + 0.5 * r), F32(c[a] + 1.5 * r))
                    out.append(self.bisect(h, m, a, test, "S behind, %s" % kind))
            # a float either side of far_t, from outside
            for d in dirs:
                o = (c - 3.0 * r * d).astype(F32).astype(np.float64)
                d32 = norm32(d)[0].astype(np.float64)
                b, cc = np.dot(o - c, d32), np.dot(o - c, o - c) - r * r
                far = -b + np.sqrt(max(b * b - cc, 0.0))
                for k in (-1, 0, 1):
                    out.append(rays(o, d, 0.0, ts.step(F32(far), k)))
            # origins inside, on the surface, at the centre
            v = ts._sphere(rng, 24)
            out.append(rays(c + 0.6 * r * v[:8], ts._sphere(rng, 8)))
            out.append(rays(c + r * v[8:16], ts._sphere(rng, 8)))
            out.append(rays(c + r * v[16:24], -v[16:24] + 0.3 * ts._sphere(rng, 8)))
            out.append(rays(np.tile(c, (6, 1)), AXES))
            out.append(rays(np.tile(c, (4, 1)), OBLIQUE))
            # l . d == 0 exactly: d along an axis (a coordinate of the origin equals the centre's), and d = (1, 1, 0) / sqrt 2 with l = (a, -a, b)
            c32 = c.astype(F32).astype(np.float64)
            for scale in (0.5, 0.999, 1.001, 2.0):
                out.append(rays(c32 + scale * r * np.array([0.0, 0.6, 0.8]), AXES[0]))
                a = float(F32(scale * r * 0.5))
                o = c32 + np.array([a, -a, float(F32(scale * r * 0.70710678))])
                if np.array_equal(o.astype(F32).astype(np.float64) - c32, o - c32):      # (the offsets survive the rounding of the origin)
                    out.append(rays(o, [1.0, 1.0, 0.0]))
            self.add("S", np.concatenate(out), pi)

    def _shape_record(self, p):
        fs = self.osc.flat
        ob = fs.objects[p.obj]
        return fs.shapes[(ob["index"] if ob["kind"] == 0 else fs.groups[ob["index"]]["first_shape"]) + p.shape]

    def _ident(self, p):
        """the id of a static object, read off the XML: objects are numbered in document order (a shapegroup is no object)"""
        if not hasattr(self, "_id_cache"):
            import re
            text = re.sub(r'<shape type="shapegroup".*?</shape>\s*</shape>', "", open(self.path).read(), flags=re.S)
            self._id_cache = [ident for _, ident in re.findall(r'<shape type="(\w+)"(?: id="(\w+)")?', text)]
            assert len(self._id_cache) == len(self.osc.flat.objects)
        return self._id_cache[p.obj]

    # ---- Y
    def _cylinders(self, rng):
        cyl = self.analytic(CYLINDER)
        picks = cyl[:6] + [i for i in cyl if self.prims[i].ob is not None] if self.name == "analytic_field" else cyl
        for pi in dict.fromkeys(picks):
            p = self.prims[pi]
            o_, u, v, w = p.frame()
            rad, ln = float(np.linalg.norm(u)), float(np.linalg.norm(w))
            uh, vh, wh = unit(u), unit(v), unit(w)
            test = lambda y, p=p: self.hits_prim(y, p)
            ka = int(np.argmax(np.abs(wh)))      # the world axis that runs most along the cylinder's
            out = []
            for phi in (0.3, 1.9, 3.7, 5.2):
                nrm = np.cos(phi) * uh + np.sin(phi) * vh
                side = np.cross(wh, nrm)
                # tangent to the wall: the origin slides sideways
                for dist in (3.0, 30.0):
                    d = -nrm + 0.2 * wh
                    base = rays(o_ + 0.5 * w - dist * rad * unit(d), d)
                    k = int(np.argmax(np.abs(side)))
                    s = np.sign(side[k]) or 1.0
                    h, m = self.pair(base, k, base[0, k] + F32(s * 0.3 * rad / abs(side[k])), base[0, k] + F32(s * 3.0 * rad / abs(side[k])))
                    out.append(self.bisect(h, m, k, test, "Y tangent"))
                # across both ends: the origin slides along the axis
                for z_in, z_out in ((0.2, -0.4), (0.8, 1.4)):
                    base = rays(p.at([np.cos(phi), np.sin(phi), z_in])[0] + 3.0 * rad * nrm, -nrm)
                    shift = (z_out - z_in) * ln / wh[ka]
                    h, m = self.pair(base, ka, base[0, ka], base[0, ka] + F32(shift))
                    out.append(self.bisect(h, m, ka, test, "Y end z == %d" % round(z_in)))
                # through the open end z == 0 onto the wall from inside: the near root lies before the end; slid along the axis until the far root leaves the other end
                start = o_ - 1.0 * w + 0.3 * rad * nrm
                base = rays(start, p.at([np.cos(phi + 2.5), np.sin(phi + 2.5), 0.5])[0] - start)
                h, m = self.pair(base, ka, base[0, ka], base[0, ka] + F32(1.2 * ln / wh[ka]))
                out.append(self.bisect(h, m, ka, test, "Y inside through the end"))
                out.append(base)
                # maxt around the near root (from outside) and the far root (from the axis)
                for start, d in ((o_ + 0.5 * w + 3.0 * rad * nrm, -nrm + 0.1 * wh), (o_ + 0.5 * w, nrm + 0.1 * wh)):
                    h, m = self.pair(rays(start, d), 7, FMAX, 0.0)
                    out.append(self.bisect(h, m, 7, test, "Y maxt"))
            # parallel to the axis: inside, on the wall, outside; both directions
            for rho in (0.0, 0.5, 1.0, 2.0):
                for sgn in (1.0, -1.0):
                    out.append(rays(p.at([rho, 0.0, 0.5 - 1.5 * sgn])[0], sgn * w))
            # the cylinder behind the origin (far_t < 0); origins on the axis
            out.append(rays(o_ + 0.5 * w + 3.0 * rad * uh, [uh + 0.1 * wh, uh - 0.3 * vh]))
            out.append(rays(np.tile(o_ + 0.5 * w, (4, 1)), OBLIQUE))
            out.append(rays(np.tile(o_ + 0.5 * w, (6, 1)), AXES))
            self.add("Y", np.concatenate(out), pi)

    # ---- K
    def _disks(self, rng):
        dk = self.analytic(DISK)
        picks = dk[:7] + [i for i in dk if self.prims[i].ob is not None] if self.name == "analytic_field" else dk
        for pi in dict.fromkeys(picks):
            p = self.prims[pi]
            o_, u, v, w = p.frame()
            rad = float(np.linalg.norm(u))
            wh = unit(w)
            test = lambda y, p=p: self.hits_prim(y, p)
            kn = int(np.argmax(np.abs(wh)))
            out = []
            for j in range(8):      # the rim
                th = 2 * np.pi * (j + 0.37) / 8
                radial = unit(np.cos(th) * u + np.sin(th) * v)
                k = int(np.argmax(np.abs(radial)))
                for d in (-wh + 0.3 * radial, wh + 0.2 * np.cross(wh, radial)):
                    base = rays(o_ + 0.5 * rad * radial - 2.0 * rad * unit(d), d)
                    h, m = self.pair(base, k, base[0, k], base[0, k] + F32(2.0 * rad / radial[k]))
                    out.append(self.bisect(h, m, k, test, "K rim"))
            for d in list(OBLIQUE) + list(AXES):      # the centre
                if abs(np.dot(unit(d), wh)) > 0.05:
                    out.append(rays(o_ - 2.0 * rad * unit(d), d))
            # t around 0: the origin slides through the plane; t around maxt
            for d in (-wh, -wh + 0.4 * unit(u)):
                base = rays(o_ + 0.3 * u + 0.5 * rad * wh, d)
                h, m = self.pair(base, kn, base[0, kn], base[0, kn] - F32(1.0 * rad * wh[kn] / abs(wh[kn]) / abs(wh[kn])))
                out.append(self.bisect(h, m, kn, test, "K t == 0"))
                h, m = self.pair(base, 7, FMAX, 0.0)
                out.append(self.bisect(h, m, 7, test, "K maxt"))
            # in the plane: a direction with no normal component (exactly so for the disks whose normal is a world axis), both signs of zero, in and off the plane
            for sgn in (0.0, -0.0):
                for off in (0.0, 0.25 * rad):
                    d = unit(u).copy()
                    r_ = rays(o_ - 2.0 * u + off * wh, d)
                    if abs(wh[kn]) == 1.0:
                        r_[0, 3 + kn] = sgn
                    out.append(r_)
            self.add("K", np.concatenate(out), pi)

    # ---- T
    def _ties(self):
        out = []
        for o, d in TIE_RAYS:
            o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
            for back in (0.0, 8.0, 64.0):      # (exact floats: the coordinates the ties rest on stay what they are)
                r_ = ts.rays8(o - back * d, d, 0.0, np.inf)
                r_[:, 3:6] = norm32(d)
                out.append(r_)
                r_ = r_.copy(); r_[:, 7] = FMAX
                out.append(r_)
        self.add("T", np.concatenate(out))

    def tie_classes(self):
        """{class: rays of T whose closest t the oracle finds on both primitives of that class}"""
        r = self.rays[self.family == "T"]
        res = self.osc.tree_n(r, per_prim=True)
        slot_prim = {}
        for i, p in enumerate(self.prims):
            if p.kind != MESH:
                slot_prim[p.slot] = i
        counts = {"two spheres, two objects": 0, "sphere and disk at the pole": 0, "disk over rectangle": 0, "rectangle over disk": 0, "disk over a larger rectangle in a tilted plane": 0,
                  "inside the group and outside": 0}
        for i in np.flatnonzero(res["ids"][:, 0] >= 0):
            at = [slot_prim[s] for s in np.flatnonzero(res["prim_t"][i] == res["tuv"][i, 0]) if s in slot_prim]
            ps = [self.prims[j] for j in at]
            if len(ps) < 2:
                continue
            kinds = sorted(p.kind for p in ps)
            grouped = [p.ob is not None for p in ps]
            if any(grouped) and not all(grouped):
                counts["inside the group and outside"] += 1
            elif kinds == [SPHERE, SPHERE]:
                counts["two spheres, two objects"] += 1
            elif kinds == [SPHERE, DISK]:
                counts["sphere and disk at the pole"] += 1
            elif kinds == [RECT, DISK]:
                disk, rect = (ps[0], ps[1]) if ps[0].kind == DISK else (ps[1], ps[0])
                counts["disk over rectangle" if disk.obj < rect.obj else "rectangle over disk"] += 1
                if disk.obj < rect.obj and abs(unit(disk.W)[2]) < 0.99:
                    counts["disk over a larger rectangle in a tilted plane"] += 1
        return counts

    # ---- G
    def _instances(self, rng):
        movers = [i for i, p in enumerate(self.prims) if p.moving()]
        if not movers:
            return
        per = max(1, (40 if self.small else 600) // len(movers))
        if len(movers) > 100:
            movers, per = list(rng.choice(movers, 40 if self.small else 150, replace=False)), 1 if self.small else 3
        out = []
        for pi in movers:
            p = self.prims[pi]
            for j in range(per):
                q = p.surface(rng, 1)
                p0, p1 = p.at(q, 0.0)[0], p.at(q, SHUTTER)[0]
                move = unit(p1 - p0)
                side = 1.0 if j % 2 else -1.0
                o = p0 - side * (2.0 + rng.uniform()) * p.size * move + 0.3 * p.size * rng.normal(size=3)
                between = 0.5 * (np.linalg.norm(p0 - o) + np.linalg.norm(p1 - o))
                for time in (0.0, SHUTTER, 0.5 * SHUTTER):
                    out.append(rays(o, p0 - o, time, np.inf))
                    out.append(rays(o, p0 - o, time, between))
        self.add("G", np.concatenate(out))

    # ---- M
    def _misses(self, rng, cnt=256):
        c, r = 0.5 * (self.lo + self.hi), np.linalg.norm(self.hi - self.lo)
        out_dir = ts._sphere(rng, cnt)
        o = c + (300.0 + 100.0 * rng.uniform(size=(cnt, 1))) * max(r, 2.5) * out_dir      # (beyond the shapes around 100 too)
        self.add("M", rays(o, out_dir + 0.2 * rng.normal(size=(cnt, 3)), ts._times(rng, cnt), 1.0))

    # ---- C
    def _maxt(self, rng):
        src = self.of("A", "S", "Y", "K", "T", "G")
        res = self.osc.tree_n(src)
        hit = np.flatnonzero(res["ids"][:, 0] >= 0)
        cap = 300 if self.small else 5000
        if len(hit) > cap:
            hit = np.sort(rng.choice(hit, cap, replace=False))
        out = []
        for k in (-1, 0, 1):
            y = src[hit].copy(); y[:, 7] = ts.step(res["tuv"][hit, 0], k); out.append(y)
        self.add("C", np.concatenate(out))

    # ---- H
    def _extreme(self, rng):
        a = self.of("A")
        res = self.osc.tree_n(a)
        base = a[res["ids"][:, 0] >= 0][:3 if self.small else 6].copy()
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
            x = base.copy()
            if col is None:
                x[:, 0:3] = 1e30
            else:
                x[:, col] = 1e30 if col != 1 else -1e30
            bad.append(x)
        away = self.of("M")[:4 if self.small else 12].copy()
        away[:, 7] = np.inf
        for length in (1e-30, 1e30, 1e38):
            x = away.copy()
            with np.errstate(over="ignore"):
                x[:, 3:6] = (x[:, 3:6].astype(np.float64) * length).astype(F32)
            bad.append(x)
        for val in (np.nan, np.inf, -np.inf):
            x = away.copy(); x[:, 6] = val; bad.append(x)
        if any(f == "G" for f, _, _ in self.parts):
            g = self.of("G")
            g = g[np.isfinite(g[:, 7])][:60 if self.small else 300]
            for val in (np.nan, np.inf, -np.inf):
                x = g.copy(); x[:, 6] = val; bad.append(x)
        bad = np.concatenate(bad)
        w = self.osc.tree_n(bad)
        keep = (w["ids"][:, 0] < 0) & (w["occluded"] == 0)      # sent only where the oracle misses
        self.extreme_rays = (len(bad), int(keep.sum()))
        self.add("H", bad[keep])

    # ---- the third placement
    def _short_lists(self):
        """{label: indices into self.rays}: lists of 1, 63, 64, 65 rays and of waves * 64 - 1, waves * 64, waves * 64 + 1, certain misses (M) around ONE ray that hits"""
        miss = np.flatnonzero(self.family == "M")
        ids = self.want["ids"]
        hits = np.flatnonzero((self.family == "A") & (ids[:, 0] >= 0) & (self.want["occluded"] == 1))
        kinds = np.array([self.prims[self.by_id[(int(o), int(s))]].kind for o, s in ids[hits, 0:2]])
        hit = np.concatenate([hits[kinds == k][:1] for k in np.unique(kinds)])
        self.short = {}
        sizes = [(1, 0), (63, 17), (64, 40), (64, 63), (65, 64)]
        if any(f >= 2 for f, _ in self.forms):
            sizes += [(w * 64 + e, at) for w in WAVES for e, at in ((-1, w * 64 - 2), (0, 64 * (w - 1) + 5), (1, w * 64))]
        for k, h in enumerate(hit):
            for n, at in sizes:
                rows = miss[(np.arange(n) + 7 * k) % len(miss)].copy()
                rows[at] = h
                self.short["hit %d (%s): %d rays, the hit in lane %d" % (k, KIND_NAMES[int(kinds[list(hits).index(h)])], n, at)] = rows


# ---------------------------------------------------------------------------- what the analytic tests decide, in float64 numpy (classification only)
def decisions(sweep):
    """{decision: [rays on the one side, rays on the other]} over the rays of S, Y and K, each evaluated against the shape it was built around with the formulas of
    sphere_hit / cylinder_hit / disk_hit in float64.  It counts sides; it is no reference for the answers."""
    out = {}

    def count(key, cond):
        c = out.setdefault(key, [0, 0])
        c[0] += int(np.count_nonzero(cond)); c[1] += int(np.count_nonzero(~cond))

    fs = sweep.osc.flat
    for fam in ("S", "Y", "K"):
        for pi in np.unique(sweep.aim[sweep.family == fam]):
            p = sweep.prims[pi]
            r = sweep.rays[(sweep.family == fam) & (sweep.aim == pi)].astype(np.float64)
            o, d, maxt = r[:, 0:3], r[:, 3:6], r[:, 7]
            if p.ob is not None:
                inv = np.linalg.inv(ts.Geometry.matrix(p.ob, 0.0))
                o, d = o @ inv[:3, :3].T + inv[:3, 3], d @ inv[:3, :3].T
            ob = fs.objects[p.obj]
            sh = fs.shapes[(ob["index"] if ob["kind"] == 0 else fs.groups[ob["index"]]["first_shape"]) + p.shape]
            with np.errstate(all="ignore"):
                if fam == "S":
                    c, rad = p.O, np.linalg.norm(p.U)
                    l = o - c
                    plane_t = -(l * d).sum(1) / np.sqrt((d * d).sum(1))
                    count("S plane_t == 0", plane_t == 0)
                    count("S plane_t == 0 and no coordinate equals the centre's", (plane_t == 0) & (r[:, 0:3].astype(F32) != c.astype(F32)).all(1))
                    a, b, cc = (d * d).sum(1), 2 * (l * d).sum(1), (l * l).sum(1) - rad * rad
                    lo_, ld_ = l, d
                else:
                    m = np.asarray(sh["to_object"], np.float64).reshape(4, 4)
                    lo_, ld_ = o @ m[:3, :3].T + m[:3, 3], d @ m[:3, :3].T
                    if fam == "K":
                        t = -lo_[:, 2] / ld_[:, 2]
                        u, v = lo_[:, 0] + t * ld_[:, 0], lo_[:, 1] + t * ld_[:, 1]
                        ok = np.isfinite(t)
                        count("K ld.z == 0", ld_[:, 2] == 0)
                        count("K t >= 0", t[ok] >= 0)
                        count("K t <= maxt", t[ok & (t >= 0)] <= maxt[ok & (t >= 0)])
                        count("K u * u + v * v <= 1", (u * u + v * v)[ok & (t >= 0)] <= 1)
                        continue
                    a, b, cc = ld_[:, 0] ** 2 + ld_[:, 1] ** 2, 2 * (ld_[:, 0] * lo_[:, 0] + ld_[:, 1] * lo_[:, 1]), lo_[:, 0] ** 2 + lo_[:, 1] ** 2 - 1
                    count("Y A == 0", a == 0)
                    count("Y A == 0: C != 0 (the linear branch, b == 0: -c / 0)", cc[a == 0] != 0)
                    count("Y A == 0: C == 0 (on the wall: 0 / 0)", cc[a == 0] == 0)
                disc = b * b - 4 * a * cc
                count(fam + " discrim >= 0", disc[a != 0] >= 0)
                q = (a != 0) & (disc >= 0)
                sq = np.sqrt(np.where(q, disc, 0))
                near, far = (-b - sq) / (2 * a), (-b + sq) / (2 * a)
                near, far, mt = near[q], far[q], maxt[q]
                count(fam + " near_t <= maxt", near <= mt)
                count(fam + " far_t >= 0", far >= 0)
                inb = (near < 0) & (far > mt)
                count(fam + " in_bounds", inb)
                count(fam + " near_t < 0 (the far root answers)", near < 0)
                if fam == "Y":
                    z0, dz = lo_[q, 2], ld_[q, 2]
                    zn, zf = z0 + dz * near, z0 + dz * far
                    count("Y z_near >= 0", zn >= 0); count("Y z_near <= 1", zn <= 1); count("Y z_far >= 0", zf >= 0); count("Y z_far <= 1", zf <= 1)
                    near_ok, far_ok = (zn >= 0) & (zn <= 1) & (near >= 0), (zf >= 0) & (zf <= 1) & (far <= mt)
                    live = (near <= mt) & (far >= 0) & ~inb
                    count("Y near_ok", near_ok[live])
                    count("Y !near_ok && far_ok", (~near_ok & far_ok)[live])
    return out


def artefacts(sweep):
    """rows of the rays whose oracle hit lies on an analytic shape that the FLOAT ray, evaluated in float64, does not come near.  Nothing here reads the oracle's t, and
    nothing is added to the padding (Box::pad of scene_build.cpp per axis: 1e-5 * max(|lo|, |hi|, hi - lo) + 1e-6, on the float64 bounds of the shape at the ray's time):
      every shape   the half-line o + s d, s >= 0, meets the padded box (a float64 slab test);
      sphere        the point of the half-line closest to the centre lies within radius + pad of it;
      cylinder      the line passes the axis within radius + pad;
      disk          the point where the half-line meets the disk's plane lies within the padded box.
    (pad of a distance: the smallest of the three axes')"""
    ids = sweep.want["ids"]
    bad = []
    for i in np.flatnonzero(ids[:, 0] >= 0):
        p = sweep.prims[sweep.by_id[(int(ids[i, 0]), int(ids[i, 1]))]]
        if p.kind in (MESH, RECT):
            continue
        r = sweep.rays[i].astype(np.float64)
        o, d = r[0:3], r[3:6]
        time = min(max(r[6], 0.0), SHUTTER) if not np.isnan(r[6]) else 0.0      # (the keyframe weight clamps; its compares are false for NaN)
        lo, hi = p.bounds(time)
        pad = 1e-5 * np.maximum(np.maximum(np.abs(lo), np.abs(hi)), hi - lo) + 1e-6
        lo, hi = lo - pad, hi + pad
        with np.errstate(all="ignore"):
            t1, t2 = (lo - o) / d, (hi - o) / d
        flat = d == 0
        tn = np.where(flat, np.where((o >= lo) & (o <= hi), -np.inf, np.inf), np.minimum(t1, t2)).max()
        tf = np.where(flat, np.inf, np.maximum(t1, t2)).min()
        ok = tn <= tf and tf >= 0
        c, u, v, w = p.frame(time)
        if p.kind == SPHERE:
            x = o + max(np.dot(c - o, d) / np.dot(d, d), 0.0) * d
            ok = ok and np.linalg.norm(x - c) <= np.linalg.norm(u) + pad.min()
        elif p.kind == CYLINDER:
            n = np.cross(d, unit(w))
            dist = abs(np.dot(o - c, n)) / np.linalg.norm(n) if np.linalg.norm(n) > 0 else np.linalg.norm(np.cross(o - c, unit(w)))
            ok = ok and dist <= np.linalg.norm(u) + pad.min()
        else:
            s_ = np.dot(c - o, unit(w)) / np.dot(d, unit(w))
            x = o + s_ * d
            ok = ok and s_ >= 0 and bool(((x >= lo) & (x <= hi)).all())
        if not ok:
            bad.append(i)
    return np.array(bad, np.int64)


# ---------------------------------------------------------------------------- the device side
def device_query(mi, scene, form, waves, any_hit, r, n=None):
    """dtof_fused_query into buffers pre-filled with CANARY -> (return code, (n, 3) t, u, v as uint32 or None, ids as int32: (n, 3), or (n,) for occlusion)"""
    r = np.ascontiguousarray(r, F32).reshape(-1, 8)
    out, ids = np.full((len(r), 3), CANARY, np.uint32), np.full(len(r) if any_hit else (len(r), 3), CANARY, np.uint32)
    rc = mi._lib().dtof_fused_query(scene._h, form, waves, 1 if any_hit else 0, len(r) if n is None else n, r.ctypes.data, None if any_hit else out.ctypes.data, ids.ctypes.data)
    return rc, (None if any_hit else out), ids.view(np.int32)

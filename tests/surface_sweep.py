"""Scenes and query families of the surface-interaction sweep (test_surface_sweep_cpu.py, test_surface_sweep_gpu.py): compute_surface and offset_p of
mitsuba3dopplertof_amd/csrc/dtof_shading.h, in every form a frame's kernels run them, through dtof_surface_eval -- against the oracle's compute_si / offset_p on the
same HITS (orc_kat_surface_n).  A query is a hit, not a ray: o, d, time, t, b1, b2 and the ids object, shape in its group, face -- so t and the barycentrics can sit
where no traversal reports them.

Scenes (`forms` = the forms of dtof_surface_eval a scene meets, dtof_surface_query.h):

  analytic      a sphere, a disk and a cylinder, each plain (placed so that the pole, the centre and the axis are exact floats), with flip_normals, under a rotated,
                non-uniformly scaled to_world, and once more in a shapegroup whose instance has an animated transform of three keyframes, the second a mirror
                (negative determinant); AnimatedTransform::eval reads keyframes 0 and 1 only, so the third never shows                                        0 5
  mesh          four meshes of at most 32 faces -- vertex normals and texcoords (loaded directly AND as a moving, mirrored instance), neither, face normals with
                texcoords, and `edge` (flip_normals; faces 0: collinear uvs, det == 0; 1: det denormal, inv_det = inf; 2: vertex normals that cancel at
                b = (0.5, 0); 3: det < 0; 4: det > 0) -- and a cube                                                                                          0 5
  cornell_wall  the headline's room: four plain rectangles and the moving back wall (one-wall fact)                                                         0 1 2 3 4 5
  wall_mirror   the same room; the wall's second keyframe mirrors its own x axis, so that at the shutter's middle the instance matrix maps dp_du to the zero
                vector exactly (singular: the inverse is not finite there) and has a negative determinant behind it                                          0 1 2 3 4 5
  panel, ties_wall, wall_at_3, six, eight, ties
                the flat sweep's scenes with a memo object (tests/flat_sweep.py): a small panel for a wall; doubled rectangles; the wall at index 3 of the table;
                tables of 6, 8 and 7 objects -- what wall_frames_init's table pointer and the one-wall form's `oi == memo_obj` depend on                      0 1 2 3 4 5
  flat_pair     an axis-aligned rectangle (n = (0, 0, 1) exactly), a rotated, non-uniformly scaled one, one with flip_normals, and a moving, mirrored instance
                of a group of TWO rectangles (a memo object, no one-wall fact)                                                                               0 1 2 3 5

Families (the label of a row):

  A   reachable: rays through the oracle's own ray query (orc_kat_tree_n); t, u, v and the ids it reports become the query.  No NaN word occurs.
  B   placed by hand: per shape kind, on the compares -- see _by_hand.
  C   thresholds: for each decision orc_kat_surface_n reports, one input scanned on the oracle and every change of outcome bisected to two adjacent floats; both sent.

Layouts: in order, under a fixed permutation, and the rows of B and C alone in lists of 1, 63, 64 and 65.  Everything is a function of SEED."""
import os
import sys

import numpy as np

from conftest import SCENES

sys.path.insert(0, SCENES)
import make_mesh      # noqa: E402
import make_scenes as ms      # noqa: E402
from tree_sweep import F32, DENORM, CANARY, ordf, unordf, step, grid      # noqa: E402,F401

SEED = 20261020
SHUTTER = 0.0015
FORM_NAMES = ("mesh", "rect", "rect_memo_regs", "rect_memo_lds", "one_wall", "mesh_memo_regs")
ALL = (0, 1, 2, 3, 4, 5)
FLAT_SWEEP_SCENES = ("panel", "ties_wall", "wall_at_3", "six", "eight", "ties")      # the scenes of tests/flat_sweep.py that bring a memo object (beside `closed` = cornell_wall)
SCENE_FORMS = ([("analytic", (0, 5)), ("mesh", (0, 5)), ("cornell_wall", ALL), ("wall_mirror", ALL), ("flat_pair", (0, 1, 2, 3, 5))] +
               [(n, ALL) for n in FLAT_SWEEP_SCENES])      # (each of them meets the one-wall fact: dtof_scene_export kind 26, which the GPU module reads back)
NAMES = [n for n, _ in SCENE_FORMS]
CASES = [(n, f, w) for n, forms in SCENE_FORMS for f in forms for w in (1, 0)]
RECT, MESH, SPHERE, DISK, CYL = 0, 1, 2, 3, 4
OPS = ("disk_r", "sphere_rd", "mesh_det", "dpdu_zero", "segment", "weight", "offset_dot")
# the words of out32
P, N, SH_N, SH_S, SH_T, WI, UV, DP_DU, DP_DV, OFF_UP, OFF_DOWN = (slice(0, 3), slice(3, 6), slice(6, 9), slice(9, 12), slice(12, 15), slice(15, 18), slice(18, 20),
                                                                   slice(20, 23), slice(23, 26), slice(26, 29), slice(29, 32))
FRAME_WORDS = np.r_[9:15, 15:17, 20:26]      # sh_s, sh_t, wi.x, wi.y, dp_du, dp_dv: +0 with want_frame = 0
KEPT_WORDS = np.setdiff1d(np.arange(32), FRAME_WORDS)
DP_WORDS = np.r_[20:26]
NAN_CAP = 0.15


# ---------------------------------------------------------------------------- scenes
def _head():
    s = ms.HEADER.format(spp=4, res=16, tsm="antithetic", shift="0.5") + ms.SENSOR.format(fov="19.5", cam=ms.CAM)
    for b in ms.BSDFS:
        s += ms.bsdf(*b)
    return s


def _shape(plugin, body, to_world="", flip=False, bsdf="TallBoxBSDF", extra=""):
    tw = '<transform name="to_world">%s</transform>' % to_world if to_world else ""
    return '<shape type="%s">%s%s%s%s<ref id="%s"/></shape>\n' % (plugin, body, '<boolean name="flip_normals" value="true"/>' if flip else "", extra, tw, bsdf)


def _anim(key0, key1, key2=None):
    s = '<animation name="to_world"><transform time="0">%s</transform><transform time="0.0015">%s</transform>' % (key0, key1)
    if key2 is not None:
        s += '<transform time="0.003">%s</transform>' % key2
    return s + '</animation>'


SCALED = '<scale x="0.5" y="0.3" z="0.2"/><rotate x="1" y="1" angle="35"/>'


def _edge_mesh():
    """five triangles with vertices of their own in the plane z = 0 (see the module's text) -> (positions, normals, uvs, faces)"""
    pos, nrm, uv, faces = [], [], [], []
    up = (0.0, 0.0, 1.0)
    per_face = [
        ([(0.0, 0.0), (0.5, 0.5), (1.0, 1.0)], [up, up, up]),                                  # collinear uvs: det == 0
        ([(0.0, 0.0), (1e-20, 0.0), (0.0, 1e-20)], [up, up, up]),                              # det = 1e-40, a denormal: inv_det overflows
        ([(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)], [up, (0.0, 0.0, -1.0), (1.0, 0.0, 0.0)]),        # n0 / 2 + n1 / 2 == 0 at b = (0.5, 0)
        ([(0.0, 0.0), (0.0, 1.0), (1.0, 0.0)], [up, up, up]),                                  # det < 0
        ([(0.25, 0.125), (0.75, 0.25), (0.5, 0.875)], [(0.0, 0.6, 0.8), up, (0.6, 0.0, 0.8)]),   # det > 0
    ]
    for k, (uvs, ns) in enumerate(per_face):
        x = 1.25 * k - 2.5
        pos += [(x, 0.0, 0.0), (x + 1.0, 0.0, 0.0), (x, 1.0, 0.0)]
        uv += uvs
        nrm += ns
        faces.append((3 * k, 3 * k + 1, 3 * k + 2))
    return pos, nrm, uv, faces


def _tilted_grid(seed):
    """grid(2, .): 8 faces in the plane y = 0 with vertex normals that are not the face's"""
    pos, nrm, uv, faces = grid(2, 0.5)
    rng = np.random.default_rng([SEED, seed])
    out = []
    for n in nrm:
        v = np.asarray(n) + 0.3 * rng.normal(size=3)
        out.append(tuple(float(x) for x in (v / np.linalg.norm(v)).astype(F32)))
    return pos, out, uv, faces


def build(name, d):
    """writes the scene `name` and its meshes into the directory d -> path of the XML file"""
    d = str(d)
    if name == "cornell_wall":
        return os.path.join(SCENES, "cornell_wall.xml")
    if name in FLAT_SWEEP_SCENES:
        import flat_sweep
        path = os.path.join(d, name + ".xml")
        open(path, "w").write(flat_sweep.scene_xml(name))
        return path
    s = _head()
    if name == "analytic":
        ball = '<point name="center" x="%s" y="%s" z="%s"/><float name="radius" value="%s"/>'
        pipe = '<point name="p0" x="%s" y="%s" z="%s"/><point name="p1" x="%s" y="%s" z="%s"/><float name="radius" value="%s"/>'
        s += _shape("sphere", ball % (0, 0, 1, 0.5))                                                      # centre on the z axis: the poles are exact
        s += _shape("sphere", ball % (1.5, 0.25, 0, 0.25), flip=True)
        s += _shape("sphere", "", SCALED + '<translate x="-1.5" y="0.25" z="0.125"/>')
        s += _shape("disk", "", '<scale value="0.5"/><translate x="0" y="1.5" z="0"/>', bsdf="ShortBoxBSDF")
        s += _shape("disk", "", '<scale value="0.25"/><rotate x="1" angle="-70"/><translate x="1.5" y="1.5" z="0"/>', flip=True, bsdf="ShortBoxBSDF")
        s += _shape("disk", "", SCALED + '<translate x="-1.5" y="1.5" z="0"/>', bsdf="ShortBoxBSDF")
        s += _shape("cylinder", pipe % (0, -1.5, -0.25, 0, -1.5, 0.25, 0.25))                             # 1 / radius = 4: the axis is exact
        s += _shape("cylinder", pipe % (1.5, -1.5, -0.25, 1.25, -1.25, 0.25, 0.2), flip=True)
        s += _shape("cylinder", "", SCALED + '<translate x="-1.5" y="-1.5" z="0"/>')
        s += ('<shape type="shapegroup" id="G">' + _shape("sphere", ball % (0, 0, 0, 0.25)) + _shape("disk", "", '<scale value="0.25"/><translate x="0.75"/>', bsdf="ShortBoxBSDF") +
              _shape("cylinder", pipe % (-0.75, 0, -0.25, -0.75, 0, 0.25, 0.2)) + '</shape>\n')
        s += ('<shape type="instance"><ref id="G"/>' + _anim('<rotate z="1" angle="20"/><translate x="0" y="0" z="-1.5"/>',
                                                            '<scale x="-0.5" y="1" z="1"/><rotate z="1" angle="20"/><translate x="0.125" y="0" z="-1.5"/>',
                                                            '<translate x="5" y="5" z="5"/>') + '</shape>\n')
    elif name == "mesh":
        make_mesh.write_ply(os.path.join(d, "vn_uv.ply"), *_tilted_grid(1), with_normals=True, with_uv=True)
        make_mesh.write_ply(os.path.join(d, "none.ply"), *grid(3, 0.5), with_normals=False, with_uv=False)
        make_mesh.write_ply(os.path.join(d, "fn_uv.ply"), *_tilted_grid(2), with_normals=True, with_uv=True)
        make_mesh.write_ply(os.path.join(d, "edge.ply"), *_edge_mesh(), with_normals=True, with_uv=True)
        ply = '<string name="filename" value="%s"/>'
        s += _shape("ply", ply % "vn_uv.ply", '<rotate x="1" angle="25"/><scale x="1.5" y="1" z="0.75"/><translate x="0" y="0" z="1.5"/>')
        s += _shape("ply", ply % "none.ply", '<rotate z="1" angle="40"/><translate x="1.5" y="0" z="0"/>')
        s += _shape("ply", ply % "fn_uv.ply", '<rotate x="1" angle="-50"/><translate x="-1.5" y="0" z="0"/>', extra='<boolean name="face_normals" value="true"/>')
        s += _shape("ply", ply % "edge.ply", "", flip=True)                                              # no to_world: the vertex normals stay what the file holds
        s += _shape("cube", "", '<scale value="0.25"/><rotate y="1" angle="30"/><translate x="0" y="-1.5" z="0"/>', bsdf="ShortBoxBSDF")
        s += ('<shape type="ply">' + ply % "vn_uv.ply" + _anim('<rotate x="1" angle="25"/><translate x="0" y="1.5" z="-1.5"/>',
                                                              '<scale x="-1" y="1" z="1.25"/><rotate x="1" angle="25"/><translate x="0" y="1.5" z="-1.375"/>') +
              '<ref id="ShortBoxBSDF"/></shape>\n')
    elif name == "wall_mirror":
        for wall, m, b in ms.WALLS:
            if wall != "BackWall":
                s += ms.rect(wall, m, b)
            else:
                mat = '<matrix value="%s"/>' % m
                s += '<shape type="rectangle" id="BackWall">' + _anim(mat, '<scale x="-1" y="1" z="1"/>' + mat + '<translate x="0" y="0" z="0.015"/>') + '<ref id="%s"/></shape>\n' % b
    elif name == "flat_pair":
        s += _shape("rectangle", "", '<scale value="0.5"/><translate x="0" y="0" z="-2"/>')
        s += _shape("rectangle", "", SCALED + '<translate x="1.5" y="0" z="0"/>')
        s += _shape("rectangle", "", '<scale value="0.5"/><rotate y="1" angle="60"/><translate x="-1.5" y="0" z="0"/>', flip=True)
        s += ('<shape type="shapegroup" id="G">' + _shape("rectangle", "", '<scale x="0.5" y="0.25"/><translate x="0" y="0.5" z="0"/>', bsdf="ShortBoxBSDF") +
              _shape("rectangle", "", '<scale x="0.25" y="0.5"/><rotate x="1" angle="40"/><translate x="0" y="-0.5" z="0"/>', flip=True, bsdf="ShortBoxBSDF") + '</shape>\n')
        s += ('<shape type="instance"><ref id="G"/>' + _anim('<rotate y="1" angle="15"/><translate x="0" y="0" z="1.5"/>',
                                                            '<scale x="-0.75" y="1" z="1"/><rotate y="1" angle="15"/><translate x="0" y="0.125" z="1.5"/>') + '</shape>\n')
    else:
        raise KeyError(name)
    path = os.path.join(d, name + ".xml")
    open(path, "w").write(s + ms.LIGHT + "</scene>\n")
    return path


# ---------------------------------------------------------------------------- the shapes of a scene
class Slot:
    """one (object, shape in its group): the oracle's shape record, its kind, the instance's object record (None for a plain shape)"""

    def __init__(self, obj, k, sh, ob):
        self.obj, self.k, self.sh, self.ob, self.kind = obj, k, sh, ob, sh["kind"]
        self.to_world = np.asarray(sh["to_world"], np.float64).reshape(4, 4)
        self.n_faces = len(sh["faces"]) // 3 if self.kind == MESH else 0

    def matrix(self, time):
        if self.ob is None:
            return np.eye(4)
        k0, k1 = (np.asarray(self.ob["key"][i], np.float64).reshape(4, 4) for i in (0, 1))
        if self.ob["n_keys"] <= 1:
            return k0
        a = min(max((time - float(self.ob["key_time"][0])) / (float(self.ob["key_time"][1]) - float(self.ob["key_time"][0])), 0.0), 1.0)
        return k0 * (1 - a) + k1 * a

    def world(self, local, time=0.0, vector=False):
        """a point (vector) of the shape's own space -- the unit sphere, disk, rectangle, cylinder -- in the world at `time`"""
        m = self.matrix(time) @ (self.to_world if self.kind != MESH else np.eye(4))
        v = m[:3, :3] @ np.asarray(local, np.float64)
        return v if vector else v + m[:3, 3]

    def centre(self, time=0.0):
        if self.kind == MESH:
            nv = len(self.sh["positions"]) // 3
            c = np.asarray(self.sh["positions"], np.float64).reshape(nv, 3).mean(0)
            m = self.matrix(time)
            return m[:3, :3] @ c + m[:3, 3]
        return self.world((0.0, 0.0, 0.5 if self.kind == CYL else 0.0), time)


def slots_of(osc):
    fs, out = osc.flat, []
    for oi, ob in enumerate(fs.objects):
        first, count = (ob["index"], 1) if ob["kind"] == 0 else (fs.groups[ob["index"]]["first_shape"], fs.groups[ob["index"]]["n_shapes"])
        for k in range(count):
            out.append(Slot(oi, k, fs.shapes[first + k], ob if ob["kind"] != 0 else None))
    return out


def fl(x):
    """the one float of a scalar or a one-element array"""
    return float(np.asarray(x).reshape(-1)[0])


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def row(o, d, time, t, b1, b2):
    r = np.zeros(10, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        r[0:3], r[3:6], r[6], r[7], r[8], r[9] = np.asarray(o, np.float64), np.asarray(d, np.float64), time, t, b1, b2
    return r


class Sweep:
    """the queries of one scene with their labels, layouts and oracle answers"""

    def __init__(self, name, orc, directory, n_random=3000):
        self.name, self.forms = name, dict(SCENE_FORMS)[name]
        self.path = build(name, directory)
        self.osc = orc.Scene(self.path, dict(resx=16, resy=16))
        self.slots = slots_of(self.osc)
        self.by_ids = {(s.obj, s.k): s for s in self.slots}
        self.q, self.ids, self.family = [], [], []
        rng = np.random.default_rng([SEED, NAMES.index(name)])
        self._reachable(rng, n_random)
        self.n_a = len(self.q)
        self._by_hand(rng)
        self._thresholds()
        self.q, self.ids = np.ascontiguousarray(np.stack(self.q), F32), np.ascontiguousarray(np.stack(self.ids), np.int32)
        self.family = np.array(self.family)
        self.n = len(self.q)
        self.want, self.ops = self.osc.surface_n(self.q, self.ids)
        self.perm = np.random.default_rng([SEED, 99]).permutation(self.n)
        bc = np.flatnonzero(self.family != "A")
        self.short = {"%d rows from %d" % (n, at): bc[(at + np.arange(n)) % len(bc)] for n, at in ((1, 0), (1, 7), (63, 3), (64, 11), (65, 2), (65, len(bc) - 30))}

    def add(self, family, q, ids):
        self.q.append(np.asarray(q, F32)); self.ids.append(np.asarray(ids, np.int32)); self.family.append(family)

    def answer(self, q, ids):
        return self.osc.surface_n(np.asarray(q, F32).reshape(-1, 10), np.asarray(ids, np.int32).reshape(-1, 3))

    # ---- A
    def _reachable(self, rng, n):
        room = self.name in ("cornell_wall", "wall_mirror") + FLAT_SWEEP_SCENES
        times = rng.uniform(0, SHUTTER, n)
        times[0::5], times[1::5] = 0.0, SHUTTER
        if room:
            o = rng.uniform((-0.9, 0.1, -0.9), (0.9, 1.9, 0.9), (n, 3))
            d = _unit(rng, n)
        else:
            o = 5.0 * _unit(rng, n)
            d = np.empty((n, 3))
            for i in range(n):
                s = self.slots[i % len(self.slots)]
                d[i] = s.centre(times[i]) + 0.25 * rng.normal(size=3) - o[i]
            d[n // 2:] /= np.linalg.norm(d[n // 2:], axis=1, keepdims=True)      # half of them of length 1
        rays = np.zeros((n, 8), F32)
        rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = o, d, times, np.inf
        res = self.osc.tree_n(rays)
        hit = np.flatnonzero(res["ids"][:, 0] >= 0)
        # a reachable hit whose record holds a NaN word (the edge mesh's face with the denormal determinant: dp_du is infinite) is a row of B: A holds none
        q = np.concatenate([rays[hit, 0:7], res["tuv"][hit]], axis=1)
        finite = ~np.isnan(self.answer(q, res["ids"][hit])[0]).any(axis=1)
        self.moved_out_of_a = res["ids"][hit][~finite]      # (test_surface_sweep_cpu.py: every one of them, kept or not, lies on that face)
        order = np.concatenate([np.flatnonzero(finite), np.flatnonzero(~finite)[:10]])      # (ten of those are kept)
        hit = hit[order]; q = q[order]; finite = finite[order]; order = np.arange(len(hit))
        self.rays_a = rays[hit][finite]
        for j in order:
            self.add("A" if finite[j] else "B", q[j], res["ids"][hit[j]])
        self.n_reached = len(hit)

    def base(self, slot):
        """a reachable query on the slot, or one made up for it"""
        for q, ids in zip(self.q[:self.n_reached], self.ids[:self.n_reached]):
            if ids[0] == slot.obj and ids[1] == slot.k:
                return q.copy(), ids.copy()
        c = slot.centre()
        return row(c + (0.3, 0.4, 2.0), (-0.3, -0.4, -2.0), 0.0, 1.0, 0.25, 0.25), np.array([slot.obj, slot.k, 0], np.int32)

    # ---- B
    def _by_hand(self, rng):
        one_up, one_down = fl(step(1.0, 1)), fl(step(1.0, -1))
        for s in self.slots:
            q0, id0 = self.base(s)

            def put(**kw):
                q, ids = q0.copy(), id0.copy()
                for key, val in kw.items():
                    if key == "face":
                        ids[2] = val
                    elif key == "o":
                        q[0:3] = np.asarray(val, np.float64)
                    elif key == "d":
                        with np.errstate(over="ignore"):
                            q[3:6] = np.asarray(val, np.float64)
                    else:
                        q[{"time": 6, "t": 7, "b1": 8, "b2": 9}[key]] = val
                self.add("B", q, ids)
                return q
            if s.kind == DISK:
                for b1, b2 in ((0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (DENORM, DENORM), (1e-30, -1e-30), (1e-23, 0.0), (3e-23, 2e-23), (1.0, 0.0), (0.0, -1.0),
                               (0.6, 0.8), (one_down, 0.0), (one_up, 0.0), (0.0, 2.0), (-3.0, 4.0), (0.3, -0.4)):
                    put(b1=b1, b2=b2)
            if s.kind == SPHERE:
                for pole in (1.0, -1.0):
                    o, d = s.world((0, 0, 2 * pole)), s.world((0, 0, -pole), vector=True)
                    put(o=o, d=d, t=1.0, time=0.0)
                    o32 = o.astype(F32)
                    for axis, moved in ((0, step(o32[0], 1)), (1, step(o32[1], -1)), (0, o32[0] + F32(DENORM)), (0, o32[0] + F32(1e-4)), (1, o32[1] - F32(1e-3)), (0, o32[0] + F32(1e-2))):
                        o2 = o32.astype(np.float64); o2[axis] = fl(moved)      # sideways by one float, a denormal (most of these records are NaN: rd or the tangent's
                        put(o=o2, d=d, t=1.0, time=0.0)                         # squared length underflows) and by amounts that leave the record finite
                for eq in ((2, 0, 0), (0, -2, 0), (-2, 0, 0)):
                    put(o=s.world(eq), d=s.world(tuple(-0.5 * x for x in eq), vector=True), t=1.0, time=0.0)
            if s.kind == CYL:
                for x in (1.0, -1.0):
                    for y in (0.0, -0.0):
                        put(o=s.world((2 * x, y, 0.5)), d=s.world((-x, 0, 0), vector=True), t=1.0, time=0.0)      # the seam
                    put(o=s.world((2 * x, 0, 0.5)), d=s.world((-x, 0, 0), vector=True), t=2.0, time=0.0)          # p ON the axis: dp_du = 0, n = normalize(0)
                put(o=s.world((2, 0.5, 0.25)), d=s.world((-1, 0, 0), vector=True), t=2.0, time=0.0)                # ... and beside it
            if s.kind == MESH:
                faces = range(s.n_faces) if s.n_faces <= 5 else (0, 1, s.n_faces - 1)
                tiny = -2.0 ** -24
                bs = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (0.25, 0.75),
                      (0.25, fl(step(0.75, 1))), (0.25, fl(step(0.75, -1))), (tiny, 0.3), (0.3, tiny), (fl(step(0.5, 1)), 0.0), (fl(step(0.5, -1)), 0.0), (0.3, 0.3)]
                for f in faces:
                    for b1, b2 in (bs[:3] if s.n_faces == 5 and f == 1 else bs):      # (the face whose inv_det is infinite: every record on it is NaN)
                        put(face=f, b1=b1, b2=b2)
            if s.kind == RECT:
                for b1, b2 in ((0.0, -0.0), (-0.0, 0.0), (1.0, -1.0), (-1.0, 1.0), (1.5, 0.25), (0.25, -3.0)):
                    put(b1=b1, b2=b2)
                for t in (0.0, DENORM, 1e30):
                    put(t=t)
                d = q0[3:6].astype(np.float64)
                for length in (1e-3, 1.0, 1e3):
                    put(d=d / np.linalg.norm(d) * length)
                for sign in (1.0, -1.0):      # d in the plane, as exactly as a float direction is: along dp_du (wi.z = +-0 where the plane is axis-aligned)
                    put(d=sign * s.world((1, 0, 0), float(q0[6]), vector=True))
            # offset_p: dot(n, d) of either sign of zero -- every product a zero of one sign, which the sum keeps
            n = self.answer(q0, id0)[0][0, N]
            zero = np.copysign(0.0, n.astype(np.float64))
            put(d=zero); put(d=-zero)
            if s.ob is not None and s.ob["n_keys"] > 1:
                keys = [float(x) for x in s.ob["key_time"][:2]] + [0.003]      # (the third keyframe's time: nothing happens there)
                for time in [t for k in keys for t in (k, fl(step(k, 1)), fl(step(k, -1)))] + [0.0, 1.0, 0.5, -1.0, 2.0, 0.5 * SHUTTER, 0.3 * SHUTTER]:
                    put(time=time)

    # ---- C
    def scan(self, q0, id0, col, lo, hi, outcome, samples=41):
        """the rows either side of every change of outcome(ops row) while input `col` runs over the floats lo .. hi"""
        grid_ = np.unique(np.linspace(int(ordf(lo)[0]), int(ordf(hi)[0]), samples).astype(np.int64))

        def at(k):
            q = q0.copy(); q[col] = fl(unordf(k))
            return q

        def cls(k):
            return outcome(self.answer(at(k), id0)[1][0])
        seen = [cls(k) for k in grid_]
        for a, b, ca, cb in zip(grid_[:-1], grid_[1:], seen[:-1], seen[1:]):
            while ca != cb and b - a > 1:
                mid = (a + b) // 2
                cm = cls(mid)
                if cm == ca:
                    a = mid
                else:
                    b, cb = mid, cm
            if ca != cb:
                self.add("C", at(a), id0); self.add("C", at(b), id0)

    def _thresholds(self):
        sign = lambda x: "nan" if np.isnan(x) else ("-0" if np.signbit(x) else "+0") if x == 0 else ("neg" if x < 0 else "pos")      # noqa: E731
        for s in self.slots:
            q0, id0 = self.base(s)
            if s.kind == DISK:
                q = q0.copy(); q[9] = 0.0
                self.scan(q, id0, 8, -1.0, 1.0, lambda w: sign(w[0]))                      # r == 0 | r > 0 along b1
            if s.kind == SPHERE and s.ob is None:
                o, d = s.world((0, 0, 2)), s.world((0, 0, -1), vector=True)
                q = row(o, d, 0.0, 1.0, 0.0, 0.0)
                for axis in (0, 1):
                    self.scan(q, id0, axis, float(q[axis]) - 1e-3, float(q[axis]) + 1e-3, lambda w: sign(w[1]))      # rd == 0 | rd > 0 across the pole
            if s.kind == CYL and s.ob is None:
                q = row(s.world((2, 0, 0.5)), s.world((-1, 0, 0), vector=True), 0.0, 2.0, 0.0, 0.0)
                self.scan(q, id0, 7, 1.5, 2.5, lambda w: w[3])                                 # dp_du == 0 | != 0 along t through the axis
            self.scan(q0, id0, 5, -2.0 * max(1.0, abs(float(q0[5]))), 2.0 * max(1.0, abs(float(q0[5]))), lambda w: sign(w[6]))      # the sign of dot(n, d) along d.z
            if s.ob is not None and s.ob["n_keys"] > 1:
                self.scan(q0, id0, 6, -1e-3, 4e-3, lambda w: "0" if w[5] == 0 else "1" if w[5] == 1 else "in")      # the keyframe weight's two clamps along time
                self.scan(q0, id0, 6, 0.0, SHUTTER, lambda w: w[3])                          # dp_du == 0 along time (wall_mirror: at the shutter's middle)

    # ---- bookkeeping
    def nan_rows(self):
        return np.isnan(self.want).any(axis=1)

    def nan_share(self):
        """(rows of A with a NaN word, share of the rows of B and C with one)"""
        bad, a = self.nan_rows(), self.family == "A"
        return int(bad[a].sum()), float(bad[~a].mean())


# ---------------------------------------------------------------------------- the device side
def device_ids(scene, ids):
    """the oracle's ids (object, shape, FACE) as dtof_surface_eval takes them: a triangle by its index in the BLAS's order (dtof_scene_export kind 27)"""
    out = np.array(ids, np.int32).reshape(-1, 3).copy()
    for (obj, k), face_of_prim in scene.triangle_order().items():
        prim_of_face = np.empty(len(face_of_prim), np.int32)
        prim_of_face[face_of_prim.astype(np.int64)] = np.arange(len(face_of_prim), dtype=np.int32)
        rows = (out[:, 0] == obj) & (out[:, 1] == k)
        out[rows, 2] = prim_of_face[out[rows, 2]]
    return out


def device_eval(mi, scene, form, want_frame, q, ids, n=None):
    """dtof_surface_eval into a buffer pre-filled with CANARY -> (return code, (n, 32) words as uint32)"""
    q, ids = np.ascontiguousarray(q, F32).reshape(-1, 10), np.ascontiguousarray(ids, np.int32).reshape(-1, 3)
    out = np.full((len(q), 32), CANARY, np.uint32)
    rc = mi._lib().dtof_surface_eval(scene._h, form, want_frame, len(q) if n is None else n, q.ctypes.data, ids.ctypes.data, out.ctypes.data)
    return rc, out


def bits(x):
    """words as bit patterns, every NaN as one pattern: two NaNs are equal, -0 and +0 differ"""
    w = np.ascontiguousarray(x, F32).view(np.uint32).copy()
    w[np.isnan(np.ascontiguousarray(x, F32))] = 0x7fc00000
    return w


def differing(a, b, words=slice(None)):
    """rows in which two (n, 32) answers differ in the given words"""
    return np.flatnonzero((bits(a)[:, words] != bits(b)[:, words]).any(axis=1))


def describe(sw, rows, first, second, what, limit=6):
    fam, cnt = np.unique(sw.family[rows], return_counts=True)
    lines = ["%s: %d of %d rows differ; by family: %s" % (what, len(rows), sw.n, ", ".join("%s %d" % (f, c) for f, c in zip(fam, cnt)))]
    for i in rows[:limit]:
        s = sw.by_ids[(int(sw.ids[i, 0]), int(sw.ids[i, 1]))]
        bad = np.flatnonzero(bits(first[i:i + 1])[0] != bits(second[i:i + 1])[0])
        lines.append("  row %d, family %s, ids %s (shape kind %d): o %s d %s time %r t %r b %r %r" % (i, sw.family[i], sw.ids[i].tolist(), s.kind, sw.q[i, 0:3].tolist(), sw.q[i, 3:6].tolist(),
                                                                                                   float(sw.q[i, 6]), float(sw.q[i, 7]), float(sw.q[i, 8]), float(sw.q[i, 9])))
        lines.append("    words %s: first %s   second %s" % (bad.tolist(), np.asarray(first, F32)[i, bad].tolist(), np.asarray(second, F32)[i, bad].tolist()))
    return "\n".join(lines)

"""Scenes and ray families of the tree sweep (test_tree_sweep_cpu.py, test_tree_sweep_gpu.py, test_box_cull.py): the TLAS / BLAS ray query -- trace_scene,
intersect_object, node_step, box_hit and slab_ray of mitsuba3dopplertof_amd/csrc/dtof_traverse.h and dtof_box_cull.h, in every form a frame's ray kernels run it, through
dtof_tree_query -- against the oracle's brute-force scene_closest / scene_occluded over the same rays (orc_kat_tree_n).

Scenes, written into a directory from scenes/make_scenes.py and scenes/make_mesh.py (`forms` = the forms of dtof_tree_query a scene meets, dtof_tree_query.h):

  slab_small   a 6 x 6 grid mesh (72 triangles: behind a BLAS) in the plane y = 0, half-extent 0.05, at the origin, and the Cornell room's area light     0 1 2 3 4
  slab_unit    the same at half-extent 1, centred at (3, 0, -2)                                                                                          0 1 2 3 4
  blobs        three blob(24, 12) meshes (552 triangles each): one static, one a moving instance, one in a shapegroup with a rectangle                   0 1 2 3 4
  ties         an 8 x 8 grid whose vertices are multiples of 1 / 8, loaded twice at the same pose (ties across objects and across the faces that share
               an edge or a vertex); a group of a rectangle and a coplanar grid (ties across shapes); a grid and a coplanar rectangle as two objects,
               in both orders                                                                                                                           0 1 2 3 4
  mixed        blobs and a sphere, a disk and a cylinder: every shape's code over half-float nodes                                                       0 4
  deep         the room of tests/test_meshes.py with its two blob(256, 130) (66 048 triangles each): a traversal stack deeper than the eight-wave
               kernels' LDS column (kLdsStack8), so their overflow array is read and written.  A few thousand rays: the oracle is brute force.            0 1 2 3 4

Ray families (the label of a ray; every ray serves both query kinds):

  A   random: origins in and around the scene's bounds, half of the directions uniform on the sphere and half towards a point of a mesh, times over the shutter and at
      its two ends, maxt inf / the largest float / random finite.  A2: rays through two meshes, so that a box is met behind a nearer hit.
  B   box rims: for every mesh, rays towards points on the triangles that touch the mesh's bounds; one component of the direction is bisected ON THE ORACLE to the
      last float that still hits the mesh, and the ray is issued a few floats either side.
  F   far: B's target points, from their extreme vertex 1e-1 .. 1e-5 of the way to the triangle's centre, from origins 10, 1e2, 1e3 and 1e4 times the mesh's extent
      away, along directions oblique to all three axes and axis-aligned, of length 1 as a renderer's are.  (The reference's sphere test expands its float64 quadratic
      around the FLOAT point o + d * ((c - o) . d / |d|), which lies near the sphere only for a unit d: with d = target - o from 1e4 extents away that point is 1e7
      away, its float rounding moves the line by units, and the oracle reports spheres the ray never comes near -- behind boxes no traversal enters.)  In `ties` also
      the tie rays from those distances.
  E   small components: directions with one or two components in {+0, -0, +-smallest denormal, +-1e-42, +-1e-39, +-1e-38, +-1e-36, +-1e-30, +-1e-20}; the origin has the
      target's own coordinate on that axis (inside the slab of the mesh, whatever its magnitude: about 0.05 in slab_small, 2 to 4 in slab_unit) and lies 0.5, 1, 5 or
      100 away along the others.
  T   (`ties`) rays straight at the vertices, edge midpoints and cell centres of the grids.
  G   instances: rays at the moving instance at both shutter ends, and with maxt between the two distances.
  C   maxt: every hit of the families above again with maxt the float below t, t itself (a miss, as the oracle says) and the float above.  C2: maxt 0, -0, the smallest
      denormal, -1.
  H   non-finite and extreme, none of which the oracle hits: NaN and +-inf in each component of origin and direction in turn, maxt NaN and -inf, a zero direction,
      origins at 1e30, each on rays that hit before the change; directions of length 1e-30, 1e30 and 1e38 on rays that point away from everything; time NaN on rays
      that fly away and, like time -inf, on rays whose maxt lets them reach the moving instance at the shutter's end only (the keyframe weight clamps, and its
      compares are false for NaN: weight 0); time +inf on rays that reach it at the start only.  An infinite direction component makes the oracle's triangle test
      report t = 0 with NaN barycentrics for triangles anywhere in the scene, and a direction of length 1e30 that flies away from a sphere makes its float64
      quadratic report a hit 1e24 away; such a ray is sent only where the oracle misses.
  M   certain misses: origins outside the bounds that fly away from them, finite maxt.

Placements: the families in order (homogeneous waves), one fixed permutation (mixed waves), and lists of 1, 63, 64 and 65 rays cut from M with ONE ray that hits.
Everything is a function of SEED."""
import os
import sys

import numpy as np

from conftest import SCENES

sys.path.insert(0, SCENES)
import make_mesh      # noqa: E402
import make_scenes as ms      # noqa: E402

F32 = np.float32
SEED = 20261019
SHUTTER = 0.0015
FMAX = float(np.finfo(np.float32).max)
DENORM = 1.4e-45
CANARY = 0x7fc0beef
KINDS = ("closest", "occlusion")
FORM_NAMES = ("float", "half_overflow", "half_overflow_tlas_lds", "defer_pair", "half_every_shape")
LDS_STACK8 = 16      # kLdsStack8 (dtof_kernels.h)
SCENE_FORMS = [("slab_small", (0, 1, 2, 3, 4)), ("slab_unit", (0, 1, 2, 3, 4)), ("blobs", (0, 1, 2, 3, 4)), ("ties", (0, 1, 2, 3, 4)), ("mixed", (0, 4)),
               ("deep", (0, 1, 2, 3, 4))]
NAMES = [n for n, _ in SCENE_FORMS]
CASES = [(n, f, k) for n, forms in SCENE_FORMS for f in forms for k in KINDS]
SMALL = [0.0, -0.0] + [s * v for v in (DENORM, 1e-42, 1e-39, 1e-38, 1e-36, 1e-30, 1e-20) for s in (1, -1)]


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


def rays8(o, d, time, maxt):
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    r = np.zeros((max(len(o), len(d)), 8), F32)
    with np.errstate(over="ignore", invalid="ignore"):
        r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7] = o, d, time, maxt
    return r


# ---------------------------------------------------------------------------- scenes
def grid(n, half, plane="y"):
    """an n x n grid of 2 n^2 triangles with half-extent `half` in the plane y = 0 (or z = 0) -> (positions, normals, uvs, faces)"""
    pos, nrm, uv, faces = [], [], [], []
    for j in range(n + 1):
        for i in range(n + 1):
            a, b = half * (2.0 * i / n - 1.0), half * (2.0 * j / n - 1.0)
            pos.append((a, 0.0, b) if plane == "y" else (a, b, 0.0))
            nrm.append((0.0, 1.0, 0.0) if plane == "y" else (0.0, 0.0, 1.0))
            uv.append((i / n, j / n))
    w = n + 1
    for j in range(n):
        for i in range(n):
            a, b, c, d = j * w + i, j * w + i + 1, (j + 1) * w + i, (j + 1) * w + i + 1
            faces += [(a, b, c), (b, d, c)]
    return pos, nrm, uv, faces


def _head(walls=False):
    s = ms.HEADER.format(spp=4, res=16, tsm="antithetic", shift="0.5") + ms.SENSOR.format(fov="19.5", cam=ms.CAM)
    for b in ms.BSDFS:
        s += ms.bsdf(*b)
    if walls:
        for name, m, b in ms.WALLS:
            s += ms.rect(name, m, b)
    return s


def _ply(tag, filename, scale, translate, bsdf="TallBoxBSDF"):
    return ('<shape type="ply"%s><string name="filename" value="%s"/><transform name="to_world"><scale value="%s"/><translate x="%s" y="%s" z="%s"/></transform>'
            '<ref id="%s"/></shape>\n' % ((' id="%s"' % tag if tag else ""), filename, scale, translate[0], translate[1], translate[2], bsdf))


BLOBS = (make_mesh.mesh_shape("ply", "StaticBlob", "blob.ply", "TallBoxBSDF", "0.38", ("-0.38", "0.45", "-0.25")) +
         make_mesh.mesh_shape("ply", "MovingBlob", "blob.ply", "ShortBoxBSDF", "0.3", ("0.4", "0.33", "0.35"), anim_dz="0.015") +
         '<shape type="shapegroup" id="G"><shape type="ply"><string name="filename" value="blob.ply"/><transform name="to_world"><scale value="0.2"/></transform>'
         '<ref id="TallBoxBSDF"/></shape><shape type="rectangle"><transform name="to_world"><scale x="0.3" y="0.08"/><rotate x="1" angle="-60"/><translate y="-0.25"/>'
         '</transform><ref id="ShortBoxBSDF"/></shape></shape>\n'
         '<shape type="instance"><ref id="G"/><transform name="to_world"><rotate y="1" angle="20"/><translate x="0.1" y="1.4" z="-0.3"/></transform></shape>\n')
ANALYTIC = (ms.sphere("Ball", "TallBoxBSDF", ("-0.5", "1.5", "0.4"), "0.25") +
            '\t<shape type="disk" id="Disk"><transform name="to_world"><scale value="0.3"/><rotate x="1" angle="-70"/><translate x="0.6" y="1.2" z="-0.5"/></transform>'
            '<ref id="ShortBoxBSDF"/></shape>\n' + ms.cylinder("Pipe", "TallBoxBSDF", ("-0.8", "0.2", "0.6"), ("-0.6", "1.0", "0.7"), "0.12"))


def build(name, d):
    """writes the scene `name` and its meshes into the directory d -> path of the XML file"""
    d = str(d)
    if name in ("slab_small", "slab_unit"):
        small = name == "slab_small"
        make_mesh.write_ply(os.path.join(d, "grid.ply"), *grid(6, 0.05 if small else 1.0))
        s = _head() + _ply("Slab", "grid.ply", "1", ("0", "0", "0") if small else ("3", "0", "-2")) + ms.AREA_LIGHT
    elif name in ("blobs", "mixed"):
        make_mesh.write_ply(os.path.join(d, "blob.ply"), *make_mesh.blob(24, 12))
        s = _head() + BLOBS + (ANALYTIC if name == "mixed" else "") + ms.LIGHT
    elif name == "ties":
        make_mesh.write_ply(os.path.join(d, "tgrid.ply"), *grid(8, 0.5))
        make_mesh.write_ply(os.path.join(d, "tgrid_z.ply"), *grid(8, 0.5, "z"))
        rect = '<shape type="rectangle"%s><transform name="to_world"><scale value="0.5"/><translate x="%s" y="%s" z="%s"/></transform><ref id="ShortBoxBSDF"/></shape>\n'
        s = (_head() + _ply("Twin0", "tgrid.ply", "1", ("0", "0.5", "0")) + _ply("Twin1", "tgrid.ply", "1", ("0", "0.5", "0"), "ShortBoxBSDF") +
             '<shape type="shapegroup" id="G">' + rect % ("", "0", "0", "0") + _ply("", "tgrid_z.ply", "1", ("0", "0", "0")) + '</shape>\n'
             '<shape type="instance"><ref id="G"/><transform name="to_world"><translate x="1.5" y="0.5" z="0"/></transform></shape>\n' +
             _ply("GridA", "tgrid_z.ply", "1", ("-1.5", "0.5", "0")) + rect % (' id="RectA"', "-1.5", "0.5", "0") +
             rect % (' id="RectB"', "0", "2", "0") + _ply("GridB", "tgrid_z.ply", "1", ("0", "2", "0")) + ms.LIGHT)
    elif name == "deep":
        pos, nrm, uv, faces = make_mesh.blob(256, 130)
        make_mesh.write_ply(os.path.join(d, "blob.ply"), pos, nrm, uv, faces)
        make_mesh.write_obj(os.path.join(d, "blob.obj"), pos, nrm, uv, faces)
        s = make_mesh.cornell_mesh_xml()[:-len("</scene>\n")]
    else:
        raise KeyError(name)
    path = os.path.join(d, name + ".xml")
    open(path, "w").write(s + "</scene>\n")
    return path


# ---------------------------------------------------------------------------- the meshes of a scene
class Geometry:
    """the triangle meshes of the oracle's scene: object, shape in its group, vertices in the object's own space, faces, the instance's keyframes (or None)"""

    def __init__(self, osc):
        fs = osc.flat
        self.meshes, self.others = [], []
        for oi, ob in enumerate(fs.objects):
            first, count = (ob["index"], 1) if ob["kind"] == 0 else (fs.groups[ob["index"]]["first_shape"], fs.groups[ob["index"]]["n_shapes"])
            for k in range(count):
                sh = fs.shapes[first + k]
                if sh["kind"] == 1:
                    nv = len(sh["positions"]) // 3
                    self.meshes.append(dict(obj=oi, shape=k, pos=np.asarray(sh["positions"], np.float64).reshape(nv, 3), faces=np.asarray(sh["faces"], np.int64).reshape(-1, 3),
                                            ob=ob if ob["kind"] != 0 else None))
                else:
                    self.others.append((oi, k))
        allp = np.concatenate([self.world(m, 0.0) for m in self.meshes])
        self.lo, self.hi = allp.min(0), allp.max(0)

    @staticmethod
    def matrix(ob, time):
        if ob is None:
            return np.eye(4)
        k0, k1 = np.asarray(ob["key"][0], np.float64).reshape(4, 4), np.asarray(ob["key"][1], np.float64).reshape(4, 4)
        if ob["n_keys"] <= 1:
            return k0
        a = min(max((time - float(ob["key_time"][0])) / (float(ob["key_time"][1]) - float(ob["key_time"][0])), 0.0), 1.0)
        return k0 * (1 - a) + k1 * a

    def world(self, m, time, pts=None):
        p = m["pos"] if pts is None else np.asarray(pts, np.float64).reshape(-1, 3)
        mat = self.matrix(m["ob"], time)
        return p @ mat[:3, :3].T + mat[:3, 3]

    def moving(self):
        return [m for m in self.meshes if m["ob"] is not None and m["ob"]["n_keys"] > 1]


def _sphere(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _times(rng, n):
    t = rng.uniform(0, SHUTTER, n)
    t[0::5] = 0.0
    t[1::5] = SHUTTER
    return t


def _maxts(rng, n, scale):
    pick = rng.integers(0, 3, n)
    return np.where(pick == 0, np.inf, np.where(pick == 1, FMAX, rng.uniform(0.0, 3.0 * scale, n)))


OBLIQUE = np.array([[0.61, 0.53, 0.59], [-0.48, 0.71, 0.52], [0.55, -0.62, -0.56], [-0.7, -0.45, 0.55]])
AXES = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])


class Sweep:
    """the rays of one scene with their labels, placements and oracle answers"""

    def __init__(self, name, orc, directory, budget=None):
        self.name, self.forms = name, dict(SCENE_FORMS)[name]
        self.path = build(name, directory)
        self.osc = orc.Scene(self.path, dict(resx=16, resy=16))
        self.geo = Geometry(self.osc)
        self.small = name == "deep"      # the oracle is brute force over 132 096 triangles: a few thousand rays in all
        self.parts, self.targets = [], []
        rng = np.random.default_rng([SEED, NAMES.index(name)])
        self.extent = float((self.geo.hi - self.geo.lo).max())
        self._random(rng, 160 if self.small else 4000)
        self._rims(rng)
        self._far(rng)
        self._small_components(rng)
        if name == "ties":
            self._ties(rng)
        self._instances(rng)
        self._misses(rng)
        self._maxt(rng)      # (behind the families it repeats)
        self._extreme(rng)
        self.rays = np.ascontiguousarray(np.concatenate([r for _, r in self.parts]))
        self.family = np.concatenate([np.full(len(r), f, dtype="U2") for f, r in self.parts])
        self.n = len(self.rays)
        self.perm = np.random.default_rng([SEED, 99]).permutation(self.n)
        self.want = self.osc.tree_n(self.rays)
        self._short_lists()

    def add(self, family, rays):
        if len(rays):
            self.parts.append((family, np.ascontiguousarray(rays, F32).reshape(-1, 8)))

    def of(self, *families):
        return np.concatenate([r for f, r in self.parts if f in families])

    def hits_mesh(self, rays, m):
        return self.osc.tree_n(rays)["ids"][:, 0] == m["obj"]

    # ---- A, A2
    def _random(self, rng, n):
        g = self.geo
        pad = 0.6 * (g.hi - g.lo) + 0.05 * self.extent
        o = rng.uniform(g.lo - pad, g.hi + pad, (n, 3))
        d = _sphere(rng, n)
        tm = _times(rng, n)
        for i in range(0, n, 2):      # every other ray towards a point of a mesh
            m = g.meshes[(i // 2) % len(g.meshes)]
            f = m["faces"][rng.integers(len(m["faces"]))]
            w = rng.dirichlet((1, 1, 1))
            d[i] = g.world(m, tm[i], w @ m["pos"][f])[0] - o[i]
        self.add("A", rays8(o, d, tm, _maxts(rng, n, self.extent)))
        through = []
        for j, a in enumerate(g.meshes):
            for k, b in enumerate(g.meshes):
                if j != k:
                    cnt = 8 if self.small else 60
                    tm = _times(rng, cnt)
                    p = np.stack([g.world(a, t, a["pos"][rng.integers(len(a["pos"]))])[0] for t in tm])
                    q = np.stack([g.world(b, t, b["pos"][rng.integers(len(b["pos"]))])[0] for t in tm])
                    c = 0.5 * (a["pos"].min(0) + a["pos"].max(0))
                    p = p + 0.3 * (g.world(a, 0.0, c)[0] - p)      # inside mesh a, so that the ray crosses its surface on the way to b
                    through.append(rays8(p - 1.5 * (q - p), q - p, tm, np.where(rng.integers(0, 2, cnt) == 0, np.inf, FMAX)))
        if through:
            self.add("A2", np.concatenate(through))

    # ---- B: the triangles that touch the mesh's bounds
    def _rim_targets(self, rng, m, per_side):
        """[(extreme vertex, centre of a triangle that holds it, axis)] in the object's own space"""
        out = []
        lo, hi = m["pos"].min(0), m["pos"].max(0)
        for axis in range(3):
            for bound in (lo[axis], hi[axis]):
                verts = np.flatnonzero(m["pos"][:, axis] == bound)
                for v in rng.permutation(verts)[:per_side]:
                    fs_ = np.flatnonzero((m["faces"] == v).any(axis=1))
                    f = m["faces"][fs_[rng.integers(len(fs_))]]
                    out.append((m["pos"][v], m["pos"][f].mean(0), axis))
        return out

    def _rims(self, rng):
        g = self.geo
        rims = []
        for m in g.meshes:
            tg = self._rim_targets(rng, m, 1 if self.small else 3)
            size = float((m["pos"].max(0) - m["pos"].min(0)).max()) * (np.linalg.norm(g.matrix(m["ob"], 0.0)[:3, 0]))
            for v, c, axis in tg:
                self.targets.append((m, v, c, axis, size))
                p = g.world(m, 0.0, v + 0.02 * (c - v))[0]
                for dirn in OBLIQUE[:1 if self.small else 2]:
                    for back in (2.5, 0.8, 0.25):      # (from as far as nothing else is in the way: the room's walls, another mesh)
                        o = p - back * size * dirn / np.linalg.norm(dirn)
                        base = rays8(o, p - o, 0.0, np.inf)
                        if self.hits_mesh(base, m)[0]:
                            break
                    comp = 3 + int(np.argmin(np.abs(base[0, 3:6])))
                    for sign in (1.0, -1.0):
                        far = base.copy()
                        far[0, comp] = base[0, comp] + sign * 4.0 * np.abs(base[0, 3:6]).max()
                        if not self.hits_mesh(base, m)[0] or self.hits_mesh(far, m)[0]:
                            continue
                        lo_, hi_ = int(ordf(base[0, comp])[0]), int(ordf(far[0, comp])[0])
                        while abs(hi_ - lo_) > 1:      # the last float of that component with which the ray still hits the mesh
                            mid = (lo_ + hi_) // 2
                            y = base.copy(); y[0, comp] = float(unordf(mid))
                            lo_, hi_ = (mid, hi_) if self.hits_mesh(y, m)[0] else (lo_, mid)
                        for k in range(-3, 4):
                            y = base.copy(); y[0, comp] = float(unordf(lo_ - k * int(np.sign(hi_ - lo_))))
                            rims.append(y)
        self.add("B", np.concatenate(rims))

    # ---- F
    def _far(self, rng):
        g, out = self.geo, []
        dists = (10.0, 1e2, 1e3, 1e4)
        for m, v, c, axis, size in self.targets:
            for inset in (1e-1, 1e-3, 1e-5) if self.small else (1e-1, 1e-2, 1e-3, 1e-4, 1e-5):
                p = g.world(m, 0.0, v + inset * (c - v))[0]
                dirs = list(OBLIQUE[:1 if self.small else 4]) + [AXES[2 * axis], AXES[2 * axis + 1]]
                for dirn in dirs:
                    dirn = dirn / np.linalg.norm(dirn)
                    for dist in dists[::2] if self.small else dists:
                        o = (p - dist * size * dirn).astype(F32).astype(np.float64)      # the float origin first: the direction then aims from where the ray really starts
                        out.append(rays8(o, (p - o) / np.linalg.norm(p - o), 0.0, np.inf))
        self.add("F", np.concatenate(out))

    # ---- E
    def _small_components(self, rng):
        g, out = self.geo, []
        per_mesh = 2 if self.small else 10
        for m in g.meshes:
            for f in m["faces"][rng.permutation(len(m["faces"]))[:per_mesh]]:
                tri = g.world(m, 0.0, m["pos"][f])
                p = tri.mean(0)
                nrm = np.cross(tri[1] - tri[0], tri[2] - tri[0])
                j = int(np.argmax(np.abs(nrm)))      # the ray runs along the axis the triangle faces
                k, l_ = (j + 1) % 3, (j + 2) % 3
                for ci, c in enumerate(SMALL):
                    for two in (False, True):
                        if two and (ci + int(f[0])) % 4:      # a quarter of them with a second small component
                            continue
                        d = np.zeros(3)
                        d[j] = 1.0 if (ci + int(two)) % 2 else -1.0
                        d[k] = c
                        d[l_] = SMALL[(ci * 5 + 3) % len(SMALL)] if two else 0.25 * (1 if ci % 3 else -1)
                        lean = np.where(np.abs(d) < 1e-10, 0.0, d)
                        length = (0.5, 1.0, 5.0, 100.0)[(ci + int(f[1])) % 4]
                        out.append(rays8(p - length * lean, d, 0.0, np.inf if ci % 2 else FMAX))
        self.add("E", np.concatenate(out))

    # ---- T
    def _ties(self, rng):
        g, out, far = self.geo, [], []
        for m in g.meshes:
            tri = m["pos"][m["faces"]]
            pts = np.concatenate([m["pos"], 0.5 * (tri[:, 0] + tri[:, 1]), 0.5 * (tri[:, 1] + tri[:, 2]), tri.mean(1)])
            nrm = np.cross(tri[0, 1] - tri[0, 0], tri[0, 2] - tri[0, 0])
            axis = int(np.argmax(np.abs(nrm)))
            pw = g.world(m, 0.0, pts)
            for sign in (1.0, -1.0):
                d = np.zeros(3); d[axis] = -sign
                o = pw.copy(); o[:, axis] += sign * 1.0
                out.append(rays8(o, d, 0.0, np.inf))
                for dist in (10.0, 1e2, 1e3, 1e4):
                    o = pw[::7].copy(); o[:, axis] += sign * dist
                    far.append(rays8(o, d, 0.0, FMAX))
        self.add("T", np.concatenate(out))
        self.add("F", np.concatenate(far))

    # ---- G
    def _instances(self, rng):
        g, out = self.geo, []
        for m in g.moving():
            cnt = 10 if self.small else 150
            for i in range(cnt):
                f = m["faces"][rng.integers(len(m["faces"]))]
                w = rng.dirichlet((1, 1, 1)) @ m["pos"][f]
                p0, p1 = g.world(m, 0.0, w)[0], g.world(m, SHUTTER, w)[0]
                move = p1 - p0
                side = 1.0 if i % 2 else -1.0      # the instance moves away from the origin, or towards it: the finite maxt reaches it at one shutter end only
                o = p0 - side * (1.0 + rng.uniform()) * self.extent * (move / np.linalg.norm(move)) + 0.02 * self.extent * rng.normal(size=3)
                for time in (0.0, SHUTTER):
                    out.append(rays8(o, p0 - o, time, np.inf))
                    out.append(rays8(o, (p0 - o) / np.linalg.norm(p0 - o), time, 0.5 * (np.linalg.norm(p0 - o) + np.linalg.norm(p1 - o))))
        if out:
            self.add("G", np.concatenate(out))

    # ---- M
    def _misses(self, rng, cnt=256):
        g, cnt = self.geo, 96 if self.small else cnt
        c, r = 0.5 * (g.lo + g.hi), np.linalg.norm(g.hi - g.lo)
        out_dir = _sphere(rng, cnt)
        o = c + (40.0 + 20.0 * rng.uniform(size=(cnt, 1))) * max(r, 2.5) * out_dir
        d = out_dir + 0.2 * rng.normal(size=(cnt, 3))
        self.add("M", rays8(o, d, _times(rng, cnt), 1.0))

    # ---- C, C2
    def _maxt(self, rng):
        src = self.of("A", "A2", "B", "F", "E", "T", "G")
        if self.small:
            src = src[rng.permutation(len(src))[:150]]
        res = self.osc.tree_n(src)
        hit = np.flatnonzero(res["ids"][:, 0] >= 0)
        if len(hit) > 6000:
            hit = np.sort(rng.choice(hit, 6000, replace=False))
        t = res["tuv"][hit, 0]
        out = []
        for k in (-1, 0, 1):
            y = src[hit].copy(); y[:, 7] = step(t, k); out.append(y)
        self.add("C", np.concatenate(out))
        base = src[hit[:: max(1, len(hit) // (30 if self.small else 150))]]
        special = []
        for val in (0.0, -0.0, DENORM, -1.0):
            y = base.copy(); y[:, 7] = val; special.append(y)
        self.add("C2", np.concatenate(special))

    # ---- H
    def _extreme(self, rng):
        a = self.of("A")
        res = self.osc.tree_n(a)
        base = a[res["ids"][:, 0] >= 0][:2 if self.small else 6].copy()
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
            x[:, 0:3] = 1e30 if col is None else x[:, 0:3]
            if col is not None:
                x[:, col] = 1e30 if col != 1 else -1e30
            bad.append(x)
        away = self.of("M")[:4 if self.small else 12].copy()
        away[:, 7] = np.inf
        for length in (1e-30, 1e30, 1e38):
            x = away.copy()
            with np.errstate(over="ignore"):
                x[:, 3:6] = (x[:, 3:6].astype(np.float64) * length / np.linalg.norm(x[:, 3:6].astype(np.float64), axis=1, keepdims=True)).astype(F32)
            bad.append(x)
        for val in (np.nan, np.inf, -np.inf):
            x = away.copy(); x[:, 6] = val; bad.append(x)
        if "G" in [f for f, _ in self.parts]:
            # pairs (time 0, time T) of one ray whose finite maxt lets it reach the moving instance at one end only: the ray that misses, with the time past its own
            # end of the shutter (the keyframe weight clamps), and, for the one at time 0, with time NaN (the clamp's compares are false: weight 0)
            gr = self.of("G")
            hit = self.osc.tree_n(gr)["ids"][:, 0] >= 0
            took = {np.inf: 0, -np.inf: 0}
            for i in np.flatnonzero(gr[:, 7] != np.inf):
                twin = i + 2 if gr[i, 6] == 0.0 else i - 2
                if 0 <= twin < len(gr) and hit[i] and not hit[twin] and np.array_equal(gr[i, [0, 1, 2, 3, 4, 5, 7]], gr[twin, [0, 1, 2, 3, 4, 5, 7]]):
                    val = np.inf if gr[twin, 6] > 0 else -np.inf
                    if took[val] < 16:
                        took[val] += 1
                        for v in ((val,) if val > 0 else (val, np.nan)):
                            x = gr[twin:twin + 1].copy(); x[:, 6] = v; bad.append(x)
        bad = np.concatenate(bad)
        # An infinite direction component is outside what a triangle test means: den = U = V = inf pass `U + V <= |den|` for triangles anywhere, the oracle reports
        # t = T * (1 / inf) = 0 with u = v = NaN, and the device's slab test (id = 0) has already dropped their boxes.  Likewise a direction of length 1e30 that flies
        # away from a sphere: the reference's float64 quadratic around the FLOAT point o + d * plane_t has lost every digit and reports a hit 1e24 away, behind boxes the
        # ray never enters.  Those rays are not sent; the ones the oracle misses are.
        with np.errstate(over="ignore"):
            inf_d = np.isinf(bad[:, 3:6]).any(axis=1) | (np.abs(bad[:, 3:6]).max(axis=1) >= 1e29)
        keep = ~inf_d | (self.osc.tree_n(bad)["ids"][:, 0] < 0)
        self.inf_direction_rays = (int(inf_d.sum()), int((inf_d & keep).sum()))
        bad = bad[keep]
        self.add("H", bad)

    # ---- the third placement
    def _short_lists(self):
        """{label: indices into self.rays}: lists of 1, 63, 64, 65 rays, certain misses (M) around ONE ray that hits"""
        miss = np.flatnonzero(self.family == "M")
        ids = self.want["ids"]
        hits = np.flatnonzero((self.family == "A") & (ids[:, 0] >= 0) & (self.want["occluded"] == 1))
        hit = np.concatenate([hits[ids[hits, 0] == o][:1] for o in np.unique(ids[hits, 0])])
        self.short = {}
        for k, h in enumerate(hit):
            for n, at in ((1, 0), (63, 17), (64, 40), (64, 0), (64, 63), (65, 64), (65, 5)):
                rows = miss[(np.arange(n) + 7 * k) % len(miss)].copy()
                rows[at] = h
                self.short["hit %d: %d rays, the hit in lane %d" % (k, n, at)] = rows


# ---------------------------------------------------------------------------- the device side
def device_query(mi, scene, form, any_hit, rays, n=None):
    """dtof_tree_query into buffers pre-filled with CANARY -> (return code, (n, 3) t, u, v as uint32 or None, ids as int32: (n, 3), or (n,) for occlusion)"""
    rays = np.ascontiguousarray(rays, F32).reshape(-1, 8)
    out, ids = np.full((len(rays), 3), CANARY, np.uint32), np.full(len(rays) if any_hit else (len(rays), 3), CANARY, np.uint32)
    rc = mi._lib().dtof_tree_query(scene._h, form, 1 if any_hit else 0, len(rays) if n is None else n, rays.ctypes.data, None if any_hit else out.ctypes.data, ids.ctypes.data)
    return rc, (None if any_hit else out), ids.view(np.int32)


def want_words(sweep, any_hit, rows=slice(None)):
    """the oracle's answer in the words dtof_tree_query writes"""
    w = sweep.want
    if any_hit:
        return None, w["occluded"][rows].astype(np.int32)
    return np.ascontiguousarray(w["tuv"][rows]).view(np.uint32), np.ascontiguousarray(w["ids"][rows]).astype(np.int32)


def differing(a, b):
    """rows in which two answers (words or None, ids) differ"""
    bad = a[1] != b[1]
    bad = bad.any(axis=1) if bad.ndim == 2 else bad
    if a[0] is not None:
        bad = bad | (a[0] != b[0]).any(axis=1)
    return np.flatnonzero(bad)


def show(ans, i):
    if ans[0] is None:
        return "occluded %d" % ans[1][i]
    return "ids %s t %r u %r v %r" % ((ans[1][i].tolist(),) + tuple(float(x) for x in ans[0][i].view(np.float32)))


def describe(sweep, rows, got, want, what, limit=8):
    fam, cnt = np.unique(sweep.family[rows], return_counts=True)
    lines = ["%s: %d of %d rays differ; by family: %s" % (what, len(rows), sweep.n, ", ".join("%s %d" % (f, c) for f, c in zip(fam, cnt)))]
    for i in rows[:limit]:
        lines.append("  ray %d, family %s: o %s d %s time %r maxt %r" % (i, sweep.family[i], sweep.rays[i, 0:3].tolist(), sweep.rays[i, 3:6].tolist(), float(sweep.rays[i, 6]), float(sweep.rays[i, 7])))
        lines.append("    first %s   second %s" % (got(i), want(i)))
    return "\n".join(lines)


def tie_classes(sweep, rays):
    """(cross-object, cross-shape, cross-face) counts of the rays whose closest t the oracle finds on two primitives, by brute force over every primitive's own t"""
    r = sweep.osc.tree_n(rays, per_prim=True)
    pt, pid, best = r["prim_t"], r["prim_ids"], r["tuv"][:, 0]
    counts = [0, 0, 0]
    for i in np.flatnonzero(r["ids"][:, 0] >= 0):
        at = np.flatnonzero(pt[i] == best[i])
        if len(at) < 2:
            continue
        ids = pid[at]
        counts[0] += len(np.unique(ids[:, 0])) > 1
        counts[1] += any(len(np.unique(ids[ids[:, 0] == o][:, 1])) > 1 for o in np.unique(ids[:, 0]))
        counts[2] += any(len(ids[(ids[:, 0] == o) & (ids[:, 1] == s)]) > 1 for o, s in {(int(a), int(b)) for a, b, _ in ids})
    return tuple(counts)


# ---------------------------------------------------------------------------- records for the host check of the cull (tests/box_cull_check.cpp)
ISSUE_CASES = [((5.0, 5.0, -3.0), (dx, 0.25, 1.0), (0.0, 0.0, 0.0), (10.0, 10.0, 10.0)) for dx in SMALL]


def cull_records(sweep):
    """(n, 14) float32: the rays of families B, F and E that the oracle hits on a triangle, in the space of the triangle's object, each with the UNPADDED bounds of (a) that
    triangle and (b) its mesh -- the tightest and the widest box of the BLAS path to the hit"""
    g = sweep.geo
    by_ids = {(m["obj"], m["shape"]): m for m in g.meshes}
    sel = np.flatnonzero(np.isin(sweep.family, ["B", "F", "E"]))
    out = []
    for i in sel:
        obj, shape, prim = (int(x) for x in sweep.want["ids"][i])
        m = by_ids.get((obj, shape))
        if m is None:
            continue
        ray = sweep.rays[i].copy()
        if m["ob"] is not None:      # into the instance's space, as a float ray
            inv = np.linalg.inv(g.matrix(m["ob"], float(ray[6])))
            ray[0:3] = (inv[:3, :3] @ ray[0:3].astype(np.float64) + inv[:3, 3]).astype(F32)
            ray[3:6] = (inv[:3, :3] @ ray[3:6].astype(np.float64)).astype(F32)
        tri = m["pos"][m["faces"][prim]].astype(F32)
        for lo, hi in ((tri.min(0), tri.max(0)), (m["pos"].min(0).astype(F32), m["pos"].max(0).astype(F32))):
            out.append(np.concatenate([ray, lo, hi]).astype(F32))
    return np.stack(out) if out else np.zeros((0, 14), F32)


def issue_records():
    return np.array([list(o) + list(d) + [0.0, np.inf] + list(lo) + list(hi) for o, d, lo, hi in ISSUE_CASES], F32)

"""Inputs of the emitter sweep (test_emitter_sweep_cpu.py, test_emitter_sweep_gpu.py): a catalogue of small scenes and deterministic query families for the emitter side
of a path vertex -- on the device through dtof_emitter_eval (every (AREA, MESH, SPEC) level a scene can run at), in the oracle through orc_kat_emitter_n.

  mode 0 (Scene::sample_emitter_direction)   query = ref[3], e1, e2
  A  random      reference points uniform in a box of three scene diameters, draws uniform in [0, 1)
  B  edges       draws from DRAW_EDGES x DRAW_EDGES, crossed with reference points on the emitter's surface, 1 ulp off it, at its centre, on its plane (grazing), behind
                 it, in front of it and 10^4 diameters away; then 256 queries whose reference point is the very point their draws sample
  C  thresholds  queries of A and B issued again with the deciding input ON the value the oracle compared it with, and on the floats below and above.  The draws: the
                 oracle's discrete outcome (picked emitter, mesh face, row / column of the DiscreteDistribution2D, cell of the Hierarchical2D) is scanned over a grid of
                 the draw and every change is bisected down to two adjacent floats.  The reference points: moved along an arc around a spot light until cos_theta meets
                 cos_beam and cos_cutoff, along rays from a sphere's centre until dc_2 meets sqr(radius_adj) and sin_theta_max_2 meets 0.00068523, by bisection on the
                 oracle's reported operands, then stepped finely across the crossing.
  mode 1 (the emitter-hit density)           query = prev[3], hit[3], sh_n[3], u, v
  D  hit side    the sampled points of A - C as hit points, with the reference points as previous vertices and the emitter's normal (and its reverse) as the shading
                 normal; dp == 0 exactly; a previous vertex equal to the hit point; uv from family D of the BSDF sweep on the textured lights; previous vertices along
                 rays from a sphere's centre across sin_alpha == 0.99999994
  mode 2 (the environment on a miss)         query = d[3]
  E  miss side   directions uniform on the sphere, the six axes, the poles +- 1 ulp, the seam of the latitude-longitude map, centres and boundaries of texels

Everything is a function of the seed.  Every query is finite and every draw lies in [0, 1): dtof_emitter_eval refuses anything else (the table searches index by their
sample), and `valid` restates that rule for test_emitter_sweep_cpu.py."""
import os
from collections import namedtuple

import numpy as np

import bsdf_sweep as bs

F32 = np.float32
SEED = 20250317
N_A = 50000
ONE_BELOW = np.nextafter(F32(1), F32(0))
N_IN, N_OUT = {0: 5, 1: 11, 2: 3}, {0: 14, 1: 5, 2: 4}
ORC_N = {0: 49, 1: 7, 2: 4}
# the oracle's extra words (dtof_oracle.h: ORC_EMT_*)
SCALED, FACE, FACE_V, CDF_LO, CDF_HI, SY_LO, SY_HI, ROW, ROW_V, ROW_LO, ROW_HI, COL, COL_V, COL_LO, COL_HI, HIER = 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29
COS_THETA, COS_BEAM, COS_CUTOFF, DC2, RADJ2, STM2, CELL, SAMPLE_DP, DP, SIN_ALPHA = 41, 42, 43, 44, 45, 46, 47, 48, 5, 6
P, D, DIST, PDF, DELTA, WEIGHT, USABLE, INDEX = slice(0, 3), slice(3, 6), 6, 7, 8, slice(9, 12), 12, 13
OUTPUT_WORDS = {0: ("p.x", "p.y", "p.z", "d.x", "d.y", "d.z", "dist", "pdf", "delta", "weight.r", "weight.g", "weight.b", "usable", "index"),
                1: ("dist", "d.x", "d.y", "d.z", "em_pdf"), 2: ("em_pdf", "value.r", "value.g", "value.b")}
STM2_SWITCH = F32(0.00068523)
SIN_ALPHA_SWITCH = F32(0.99999994)
LEVEL_NAMES = {0: "(F,F,0)", 1: "(T,F,0)", 2: "(F,T,0)", 3: "(T,T,0)", 4: "(T,T,1)", 5: "(T,T,2)", 6: "(F,F,0)+one emitter"}

# ------------------------------------------------------------------------------------------------ the catalogue
FLOOR = '<shape type="rectangle"><transform name="to_world"><scale value="3"/><rotate x="1" angle="-90"/><translate y="-2"/></transform></shape>'
# (a <rotate> takes its axis as given, like the reference: the axes below have unit length)
SENSOR = ('<integrator type="path"/><sensor type="perspective"><float name="fov" value="40"/><film type="hdrfilm"><integer name="width" value="4"/>'
          '<integer name="height" value="4"/></film></sensor>')    # (the environment emitters take their bounding sphere when the scene is complete)
RADIANCE = '<emitter type="area"><rgb name="radiance" value="3, 5, 7"/></emitter>'
POINT_A = '<emitter type="point"><point name="position" x="0.3" y="1.2" z="-0.4"/><rgb name="intensity" value="3, 5, 7"/></emitter>'
POINT_B = '<emitter type="point"><point name="position" x="-1" y="0.5" z="2"/><rgb name="intensity" value="1, 0.5, 0.25"/></emitter>'
SPOT = ('<emitter type="spot"><transform name="to_world"><lookat origin="0, 2, 0" target="0.2, 0, 0.1" up="0, 0, 1"/></transform>'
        '<float name="cutoff_angle" value="%s"/>%s<rgb name="intensity" value="2, 4, 8"/></emitter>')
RECT_XF = '<transform name="to_world"><scale x="0.5" y="0.25" z="1"/><rotate x="0.6" y="0" z="0.8" angle="50"/><translate x="0.1" y="1.0" z="-0.2"/></transform>'
DISK_XF = '<transform name="to_world"><scale x="0.6" y="0.3" z="1"/><rotate x="1" angle="70"/><translate x="-0.2" y="0.8" z="0.3"/></transform>'
MESH_XF = '<transform name="to_world"><rotate x="0" y="0.6" z="-0.8" angle="35"/><translate x="0.4" y="0.9" z="0.1"/></transform>'
SPHERE = '<shape type="sphere"><point name="center" x="0.2" y="0.5" z="-0.3"/><float name="radius" value="0.4"/>%s' + RADIANCE + '</shape>'
SPHERE_C, SPHERE_R = np.array([0.2, 0.5, -0.3]), 0.4

# name, scene, the levels (dtof_emitter_eval) it is eligible for, the level scene_traits() implies, shapes with an emitter (mode 1), has an environment (mode 2),
# what the emitters are (family builders key on it), and a frame for the special reference points: centre, normal / axis, a tangent, diameter
Entry = namedtuple("Entry", "name xml levels traits_level hit_shapes env kind centre normal tangent diameter textured")
ALL_LEVELS = (0, 1, 2, 3, 4, 5, 6)


def _rot(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a); t = np.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


# twelve triangles in the plane z = 0: zero-area faces first, in the middle and last, areas from 2^-10 to 1 before to_world
MESH_AREAS = [0.0, 1.0, 2.0 ** -10, 0.5, 2.0 ** -7, 0.0, 0.25, 2.0 ** -3, 2.0 ** -9, 0.125, 2.0 ** -5, 0.0]


def write_mesh(path, vertex_normals):
    """the mesh light as an OBJ file: one triangle (x0, 0) (x0 + w, 0) (x0, 1) of area w / 2 per entry of MESH_AREAS, no shared vertices; with tilted per-vertex
    normals or without any.  A zero-area face is one point three times: its edge vectors are exactly 0 under any to_world.  Two equal edges are not enough: the
    cross product's fused multiply-subtract leaves a residue, and the face gets an area of 1e-9."""
    lines, x0 = [], -1.5
    for k, a in enumerate(MESH_AREAS):
        w = 2.0 * a
        if a == 0.0:
            tri = [(x0, 0.0), (x0, 0.0), (x0, 0.0)]
        else:
            tri = [(x0, 0.0), (x0 + w, 0.0), (x0, 1.0)]
        lines += ["v %r %r 0.0" % (x, y) for x, y in tri]
        if vertex_normals:
            for j in range(3):
                tilt, phi = np.radians(4 + 3 * ((k + j) % 5)), 2 * np.pi * ((3 * k + 5 * j) % 7) / 7.0
                lines.append("vn %r %r %r" % (float(np.sin(tilt) * np.cos(phi)), float(np.sin(tilt) * np.sin(phi)), float(np.cos(tilt))))
        x0 += w + 0.0625
    for k in range(len(MESH_AREAS)):
        i = 3 * k + 1
        lines.append("f %d//%d %d//%d %d//%d" % (i, i, i + 1, i + 1, i + 2, i + 2) if vertex_normals else "f %d %d %d" % (i, i + 1, i + 2))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def write_fixtures(d):
    """every file the catalogue names: the three 8 x 4 images of the BSDF sweep and the two mesh lights"""
    d = bs.write_textures(str(d))
    write_mesh(os.path.join(d, "sweep_light_n.obj"), True)
    write_mesh(os.path.join(d, "sweep_light.obj"), False)
    return d


def catalogue(d=""):
    rgb = os.path.join(d, "sweep_rgb.png")
    e = []

    def add(name, body, levels, traits_level, kind, centre, normal=(0, 1, 0), tangent=(1, 0, 0), diameter=1.0, hit_shapes=(), env=False, textured=False):
        e.append(Entry(name, '<scene version="3.0.0">%s%s%s</scene>' % (SENSOR, body, FLOOR), levels, traits_level, hit_shapes, env, kind,
                       np.asarray(centre, np.float64), np.asarray(normal, np.float64), np.asarray(tangent, np.float64), diameter, textured))

    spot_axis = np.array([0.2, -2.0, 0.1]) / np.linalg.norm([0.2, -2.0, 0.1])
    spot_t = np.cross(spot_axis, [0, 0, 1.0]); spot_t /= np.linalg.norm(spot_t)
    add("point", POINT_A, ALL_LEVELS, 0, "point", (0.3, 1.2, -0.4))
    add("two_points_and_a_spot", POINT_A + POINT_B + SPOT % ("30", ""), (4, 5), 4, "spot", (0, 2, 0), spot_axis, spot_t, 2.0)
    # 45 degrees: ON cos_theta == cos_cutoff the falloff is (cutoff - acos(cos_cutoff)) / transition, and `>` differs from `>=` only where the float32 round trip
    # acos(cos(cutoff)) falls BELOW cutoff -- it does for 45 (and 20) degrees, not for 25 .. 40, 50 or 60, where the two are the same function
    add("spot_narrow_beam", SPOT % ("45", '<float name="beam_width" value="10"/>'), (4, 5), 4, "spot", (0, 2, 0), spot_axis, spot_t, 2.0)
    add("directional", '<emitter type="directional"><vector name="direction" x="1" y="-2" z="0.5"/><rgb name="irradiance" value="1.5, 2.5, 3.5"/></emitter>', (4, 5), 4,
        "directional", (0, 0, 0), diameter=6.0)
    add("constant", '<emitter type="constant"><rgb name="radiance" value="0.5, 1, 2"/></emitter>', (4, 5), 4, "constant", (0, 0, 0), diameter=6.0, env=True)
    add("envmap", '<emitter type="envmap"><string name="filename" value="%s"/><float name="scale" value="0.6"/><transform name="to_world"><rotate x="0.6" y="0" z="0.8" angle="50"/>'
        '</transform></emitter>' % rgb, (4, 5), 4, "envmap", (0, 0, 0), diameter=6.0, env=True)
    R = _rot([0.6, 0, 0.8], 50.0)
    rect = dict(centre=(0.1, 1.0, -0.2), normal=R[:, 2], tangent=R[:, 0], diameter=1.0, hit_shapes=(0,))
    add("rectangle", '<shape type="rectangle">%s%s</shape>' % (RECT_XF, RADIANCE), (1, 3, 4, 5), 1, "rect", **rect)
    for tag, tex in (("bitmap_bilinear_repeat", bs._bitmap(rgb, "radiance", "bilinear", "repeat")), ("bitmap_nearest_mirror", bs._bitmap(rgb, "radiance", "nearest", "mirror")),
                     ("checkerboard", '<texture type="checkerboard" name="radiance"><rgb name="color0" value="0.1, 0.2, 0.3"/><rgb name="color1" value="0.9, 0.8, 0.7"/></texture>')):
        add("rectangle_" + tag, '<shape type="rectangle">%s<emitter type="area">%s</emitter></shape>' % (RECT_XF, tex), (4, 5), 4, "rect_" + tag, textured=True, **rect)
    # ... and one in a plane z = const: a reference point with the light's own z sees it under dot(d, n) == 0 exactly, where `dp < 0` alone decides a textured sample
    add("rectangle_bitmap_axis_aligned", '<shape type="rectangle"><transform name="to_world"><scale x="0.5" y="0.25" z="1"/><translate x="0.1" y="1.0" z="-0.25"/></transform>'
        '<emitter type="area">%s</emitter></shape>' % bs._bitmap(rgb, "radiance", "bilinear", "repeat"), (4, 5), 4, "rect_bitmap_axis_aligned", (0.1, 1.0, -0.25), (0, 0, 1), (1, 0, 0),
        1.0, hit_shapes=(0,), textured=True)
    Rd = _rot([1, 0, 0], 70.0)
    add("disk", '<shape type="disk">%s%s</shape>' % (DISK_XF, RADIANCE), (3, 4, 5), 3, "disk", (-0.2, 0.8, 0.3), Rd[:, 2], Rd[:, 0], 1.2, hit_shapes=(0,))
    add("sphere", SPHERE % "", (3, 4, 5), 3, "sphere", SPHERE_C, diameter=0.8, hit_shapes=(0,))
    add("sphere_flipped", SPHERE % '<boolean name="flip_normals" value="true"/>', (3, 4, 5), 3, "sphere", SPHERE_C, diameter=0.8, hit_shapes=(0,))
    Rm = _rot([0, 0.6, -0.8], 35.0)
    mesh = dict(centre=Rm @ [0.5, 0.5, 0] + [0.4, 0.9, 0.1], normal=Rm[:, 2], tangent=Rm[:, 0], diameter=5.0, hit_shapes=(0,))
    add("mesh_face_normals", '<shape type="obj"><string name="filename" value="%s"/><boolean name="face_normals" value="true"/>%s%s</shape>'
        % (os.path.join(d, "sweep_light.obj"), MESH_XF, RADIANCE), (3, 4, 5), 3, "mesh", **mesh)
    add("mesh_vertex_normals", '<shape type="obj"><string name="filename" value="%s"/>%s%s</shape>' % (os.path.join(d, "sweep_light_n.obj"), MESH_XF, RADIANCE),
        (3, 4, 5), 3, "mesh", **mesh)
    add("mixed", POINT_A + '<shape type="rectangle">%s%s</shape>' % (RECT_XF, RADIANCE) + SPHERE % ""
        + '<shape type="obj"><string name="filename" value="%s"/>%s%s</shape>' % (os.path.join(d, "sweep_light_n.obj"), MESH_XF, RADIANCE),
        (3, 4, 5), 3, "mixed", (0.2, 0.9, -0.1), diameter=5.0, hit_shapes=(0, 1, 2))
    return e


NAMES = [x.name for x in catalogue()]

# ------------------------------------------------------------------------------------------------ both sides
CANARY = bs.CANARY
same_bits = bs.same_bits


def oracle_eval(orc, osc, mode, q, shape=-1):
    """orc_kat_emitter_n: (n, N_IN[mode]) -> (n, ORC_N[mode]): the words of dtof_emitter_eval, then what the chain compared (NaN: did not run)"""
    q = np.ascontiguousarray(q, F32).reshape(-1, N_IN[mode])
    out = np.zeros((len(q), ORC_N[mode]), F32)
    import ctypes as C
    orc.lib().orc_kat_emitter_n(C.byref(osc.c), mode, shape, len(q), q.ctypes.data, out.ctypes.data)
    return out


def device_eval(mi, scene, mode, level, q, shape=-1):
    """dtof_emitter_eval into a buffer pre-filled with CANARY: (return code, (n, N_OUT[mode]) output as uint32)"""
    q = np.ascontiguousarray(q, F32).reshape(-1, N_IN[mode])
    out = np.full((len(q), N_OUT[mode]), CANARY, np.uint32)
    rc = mi._lib().dtof_emitter_eval(scene._h, mode, level, shape, len(q), q.ctypes.data, out.ctypes.data)
    return rc, out


def valid(mode, q):
    """the validation rule of dtof_emitter_eval: every float finite, the draws of mode 0 in [0, 1)"""
    q = np.asarray(q, F32)
    ok = np.isfinite(q).all()
    if mode == 0:
        ok = ok and (q[:, 3:5] >= 0).all() and (q[:, 3:5] < 1).all()
    return bool(ok)


def describe_mismatch(what, mode, family, q, got, want, versus="device vs oracle"):
    bad = ~same_bits(got, want)
    rows = np.nonzero(bad.any(axis=1))[0]
    lines = ["%s, family %s, %s: %d of %d queries differ" % (what, family, versus, len(rows), len(q))]
    for r in rows[:5]:
        lines.append("  query %d in = %s" % (r, " ".join("%08x" % w for w in np.ascontiguousarray(q[r]).view(np.uint32))))
        for c in np.nonzero(bad[r])[0]:
            lines.append("    %-10s got %08x want %08x" % (OUTPUT_WORDS[mode][c], np.asarray(got[r]).view(np.uint32)[c], np.asarray(want[r]).view(np.uint32)[c]))
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------ the families
DRAW_EDGES = np.array([0.0, bs.DENORMAL, 2.0 ** -24, np.nextafter(F32(0.5), F32(0)), 0.5, np.nextafter(F32(0.5), F32(1)), 1.0 - 2.0 ** -24], F32)


def _neighbours(x, k=2):
    """x and its k float32 neighbours on each side, kept inside [0, 1): (n, 2k + 1), flattened"""
    cols = bs._neighbours(np.asarray(x, F32).ravel(), k)
    return np.clip(cols, F32(0), ONE_BELOW).ravel()


def family_a(e, n=N_A, seed=SEED):
    rng = np.random.default_rng(seed)
    q = np.empty((n, 5), F32)
    q[:, 0:3] = (e.centre + (rng.random((n, 3)) - 0.5) * 3.0 * e.diameter).astype(F32)
    q[:, 3:5] = rng.random((n, 2), dtype=F32)
    return q


def special_points(e, surface):
    """reference points of family B: `surface` (sampled points of the emitter) and each 1 ulp off in every coordinate, the centre (a point light's position, a
    sphere's centre), points on the emitter's plane beyond its rim (grazing), behind and in front of it, and 10^4 diameters away"""
    c, n, t, dia = e.centre, e.normal, e.tangent, e.diameter
    b = np.cross(n, t)
    pts = [surface, np.nextafter(surface, F32(np.inf)), np.nextafter(surface, F32(-np.inf)), c[None].astype(F32)]
    plane = [c + dia * (r * np.cos(a) * t + r * np.sin(a) * b) for r in (0.7, 2.0, 30.0) for a in (0.0, 1.3, 2.9, 4.4)]
    pts.append(np.array(plane).astype(F32))
    pts.append(np.array([c - n * dia * s for s in (1e-3, 1.0, 50.0)] + [c + n * dia * s for s in (1e-3, 1.0, 50.0)]).astype(F32))
    far = [c + 1e4 * dia * np.array(v) / np.linalg.norm(v) for v in ((1, 0, 0), (0, -1, 0), (0.3, 0.5, -0.8), tuple(n), tuple(-n), tuple(t))]
    pts.append(np.array(far).astype(F32))
    return np.concatenate(pts)


def family_b(e, oracle0, a):
    """DRAW_EDGES x DRAW_EDGES x special_points; the surface points are what the oracle sampled for 24 queries of A"""
    s = oracle0(a[:24])[:, P]
    s = s[np.isfinite(s).all(axis=1)]
    pts = special_points(e, s)
    g1, g2 = np.meshgrid(DRAW_EDGES, DRAW_EDGES, indexing="ij")
    g = np.stack([g1.ravel(), g2.ravel()], axis=1)
    q = np.concatenate([np.repeat(pts, len(g), axis=0), np.tile(g, (len(pts), 1))], axis=1).astype(F32)
    # coincident points: the reference point IS the point its own draws sample (dist = 0: dist2 / dp is not finite, the density 0)
    co = a[24:280].copy()
    co[:, 0:3] = oracle0(co)[:, P]
    co = co[np.isfinite(co).all(axis=1)]
    return np.ascontiguousarray(np.concatenate([q, co]))


def _outcome(out):
    """the discrete choices the draws decide, NaN (did not run) as -1: picked emitter, face, row, column, cell"""
    w = out[:, [INDEX, FACE, ROW, COL, CELL]].copy()
    w[np.isnan(w)] = -1
    return w


def draw_thresholds(oracle0, ref, which, other, grid=2048):
    """every change of the outcome along draw `which` (3: e1, 4: e2), the other draw held at `other`: scanned on `grid` + 1 values, each change bisected down to two
    adjacent floats; returns those with two float32 neighbours on each side"""
    x = np.unique(np.concatenate([np.linspace(0.0, 1.0, grid, endpoint=False), [ONE_BELOW]]).astype(F32))

    def run(v):
        q = np.empty((len(v), 5), F32); q[:, 0:3] = ref; q[:, which] = v; q[:, 7 - which] = other
        return _outcome(oracle0(q))
    o = run(x)
    chg = np.nonzero((o[1:] != o[:-1]).any(axis=1))[0]
    lo, hi = x[chg].copy(), x[chg + 1].copy()
    olo = o[chg]
    while len(lo):
        li, hi_i = lo.view(np.uint32).astype(np.int64), hi.view(np.uint32).astype(np.int64)
        if (hi_i - li <= 1).all():
            break
        mid = ((li + hi_i) // 2).astype(np.uint32).view(F32)
        same = (run(mid) == olo).all(axis=1)
        lo, hi = np.where(same, mid, lo), np.where(same, hi, mid)
    return np.unique(np.concatenate([_neighbours(lo), _neighbours(hi)])) if len(lo) else np.zeros(0, F32)


def _bisect_t(pred, point, t0, t1, steps=70):
    """float64 parameters (arrays) between which pred(point(t)) changes: bisected until the interval is a few ulps of t"""
    p0 = pred(point(t0))
    for _ in range(steps):
        m = 0.5 * (t0 + t1)
        s = pred(point(m)) == p0
        t0, t1 = np.where(s, m, t0), np.where(s, t1, m)
    return t0, t1


def _across(point, t0, t1, rel=3e-8, k=24):
    """reference points stepped finely across a crossing found by _bisect_t: 2k + 1 parameters spaced rel * |t| apart around it"""
    t = 0.5 * (t0 + t1)
    steps = np.arange(-k, k + 1) * rel
    return np.concatenate([point(t * (1.0 + s)) for s in steps])


def spot_points(e, oracle0, seed):
    """reference points on arcs around the spot light across cos_theta == cos_beam and cos_theta == cos_cutoff: (azimuth, distance) pairs, the polar angle bisected"""
    rng = np.random.default_rng(seed + 3)
    n = 160
    az, r = rng.random(n) * 2 * np.pi, 10.0 ** rng.uniform(-1.0, 3.0, n)
    b = np.cross(e.normal, e.tangent)
    side = np.cos(az)[:, None] * e.tangent + np.sin(az)[:, None] * b

    def point(theta):
        return (e.centre + r[:, None] * (np.cos(theta)[:, None] * e.normal + np.sin(theta)[:, None] * side)).astype(F32)

    def run(p, col):
        q = np.zeros((len(p), 5), F32); q[:, 0:3] = p; q[:, 3] = ONE_BELOW   # e1 just below 1 picks the last emitter: the spot in both scenes
        out = oracle0(q)
        return out[:, COS_THETA] >= out[:, col] if col == COS_BEAM else out[:, COS_THETA] > out[:, col]
    pts = []
    for col in (COS_BEAM, COS_CUTOFF):
        t0, t1 = _bisect_t(lambda p: run(p, col), point, np.full(n, 1e-3), np.full(n, 1.5))
        pts.append(_across(point, t0, t1))
    return np.concatenate(pts)


def ray_points(centre, pred, lo, hi, seed, n=200):
    """points on n rays from `centre` (random directions), stepped finely across the distance in [lo, hi] at which pred(points) changes"""
    rng = np.random.default_rng(seed + 4)
    d = rng.standard_normal((n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)

    def point(t):
        return (centre + t[:, None] * d).astype(F32)
    t0, t1 = _bisect_t(pred, point, np.full(n, lo), np.full(n, hi))
    return _across(point, t0, t1)


def sphere_points(oracle0, seed, e1):
    """reference points on rays from the sphere's centre across dc_2 == sqr(radius_adj) and sin_theta_max_2 == 0.00068523 (e1 picks the sphere)"""
    def run(p):
        q = np.zeros((len(p), 5), F32); q[:, 0:3] = p; q[:, 3] = e1; q[:, 4] = 0.25
        return oracle0(q)
    r = SPHERE_R
    return np.concatenate([ray_points(SPHERE_C, lambda p: (lambda o: o[:, DC2] > o[:, RADJ2])(run(p)), 0.5 * r, 1.5 * r, seed),
                           ray_points(SPHERE_C, lambda p: np.nan_to_num(run(p)[:, STM2], nan=1.0) > STM2_SWITCH, 20 * r, 60 * r, seed + 1)])


def family_c(e, oracle0, a, b, seed=SEED):
    """see the module's docstring; {name of the deciding input: queries}"""
    out = {}
    rng = np.random.default_rng(seed + 2)
    base = np.concatenate([a[:40], b[rng.integers(0, len(b), 40)]])           # the reference points (and the other draw) the thresholds are crossed with
    ref = a[0, 0:3]
    t1 = [draw_thresholds(oracle0, ref, 3, o) for o in (a[0, 4], F32(0.1), F32(0.35), F32(0.6), F32(0.85))]   # e1: the pick, then columns / cells (one scan per row band)
    t2 = [draw_thresholds(oracle0, ref, 4, o) for o in (a[0, 3], F32(0.2), F32(0.7), F32(0.9))]                # e2: faces, rows, cells
    for name, which, ts in (("e1", 3, t1), ("e2", 4, t2)):
        qs = []
        for t, o in zip(ts, ((a[0, 4], 0.1, 0.35, 0.6, 0.85) if which == 3 else (a[0, 3], 0.2, 0.7, 0.9))):
            if not len(t):
                continue
            q = np.repeat(base, len(t), axis=0)
            q[:, which] = np.tile(t, len(base))
            half = len(q) // 2
            q[:half, 7 - which] = o                                            # half with the other draw the scan held (columns and cells depend on it), half with A's and B's own
            qs.append(q)
        if qs:
            out[name] = np.concatenate(qs)
    if e.kind == "spot":
        p = spot_points(e, oracle0, seed)
        q = np.zeros((len(p), 5), F32); q[:, 0:3] = p; q[:, 3] = ONE_BELOW; q[:, 4] = 0.5
        out["cos_theta"] = q
    if e.kind in ("sphere", "mixed"):
        e1 = F32(0.5 if e.kind == "sphere" else 0.6)                           # mixed: emitter 2 of 4 is the sphere
        p = sphere_points(oracle0, seed, e1)
        q = np.zeros((len(p), 5), F32); q[:, 0:3] = p; q[:, 3] = e1
        q[:, 4] = rng.random(len(p), dtype=F32)
        out["sphere"] = q
    return out


def family_d(e, orc_eval1, shape, samples, seed=SEED):
    """(hit, sh_n, previous vertex) from mode-0 queries and their oracle outputs `samples` = (queries, outputs) whose picked emitter sits on `shape`; see the docstring"""
    q0, o0 = samples
    ok = np.isfinite(o0[:, :7]).all(axis=1)
    q0, o0 = q0[ok][:6000], o0[ok][:6000]
    rng = np.random.default_rng(seed + 5)
    n = len(q0)
    hit, prev, d = o0[:, P], q0[:, 0:3], o0[:, D]
    # the emitter's normal at the sampled point is not an output: for a usable sample it faces the reference point, so -d tilted a little is a fair shading normal
    tilt = rng.standard_normal((n, 3)) * 0.3
    nrm = -d.astype(np.float64) + tilt
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
    uv = rng.random((n, 2), dtype=F32)
    rows = [np.concatenate([prev, hit, nrm, uv], axis=1), np.concatenate([prev, hit, -nrm, uv], axis=1)]
    # dp == 0 exactly: the normal is +z and the previous vertex shares the hit point's z
    k = min(n, 400)
    flat_prev = prev[:k].copy(); flat_prev[:, 2] = hit[:k, 2]
    z = np.tile(np.array([0, 0, 1], F32), (k, 1))
    rows.append(np.concatenate([flat_prev, hit[:k], z, uv[:k]], axis=1))
    for towards in (np.inf, -np.inf):                                          # ... and one float above / below it: dp a few 1e-8 on either side of 0
        near_prev = flat_prev.copy(); near_prev[:, 2] = np.nextafter(hit[:k, 2], F32(towards))
        rows.append(np.concatenate([near_prev, hit[:k], z, uv[:k]], axis=1))
    rows.append(np.concatenate([hit[:k], hit[:k], nrm[:k], uv[:k]], axis=1))   # the previous vertex IS the hit point
    if e.textured:
        uvd = bs.family_d()[:, 9:11]
        uvd = uvd[np.isfinite(uvd).all(axis=1)]
        j = rng.integers(0, n, len(uvd))
        rows.append(np.concatenate([prev[j], hit[j], nrm[j], uvd], axis=1))
    if e.kind in ("sphere", "mixed") and shape == (0 if e.kind == "sphere" else 1):
        # previous vertices on rays from the centre across sin_alpha == 0.99999994 (a hair outside the surface), the hit at the pole, the shading normal towards
        # the previous vertex so that dp < 0 and Sphere::pdf_direction runs
        hit0 = (SPHERE_C + np.array([0, SPHERE_R, 0])).astype(F32)

        def rows_for(p):
            m = len(p)
            to_prev = p.astype(np.float64) - hit0
            nn = to_prev / np.maximum(np.linalg.norm(to_prev, axis=1, keepdims=True), 1e-30)
            return np.concatenate([p, np.tile(hit0, (m, 1)), nn.astype(F32), np.zeros((m, 2), F32)], axis=1).astype(F32)
        p = ray_points(SPHERE_C, lambda p: np.nan_to_num(orc_eval1(rows_for(p))[:, SIN_ALPHA], nan=0.0) < SIN_ALPHA_SWITCH, 0.999 * SPHERE_R, 1.001 * SPHERE_R, seed)
        rows.append(rows_for(p))
    return np.ascontiguousarray(np.concatenate(rows).astype(F32))


def _dirs(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)


def family_e(seed=SEED, n=4000):
    """directions for the miss side: random, the axes, the poles +- 1 ulp (in every frame the catalogue's environment is rotated by), the seam, texel centres and
    boundaries of the 8 x 4 map (9 x 4 texels of m_data) in the map's own frame, rotated to the world by the catalogue's to_world"""
    rng = np.random.default_rng(seed + 6)
    R = _rot([0.6, 0, 0.8], 50.0)
    out = [_dirs(rng.standard_normal((n, 3)))]
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    out += [axes.astype(F32), (axes @ R.T).astype(F32)]
    for pole in (axes[2], axes[3], R @ axes[2], R @ axes[3]):
        p = pole.astype(F32)
        out += [np.nextafter(p, F32(np.inf))[None], np.nextafter(p, F32(-np.inf))[None], _dirs(pole + np.array([1e-7, 0, 3e-8]))[None], _dirs(pole + np.array([0, 1e-4, -1e-4]))[None]]
    # local directions from (u, v): u = atan2(x, -z) / 2 pi, v = acos(y) / pi
    us = np.unique(np.concatenate([np.arange(0, 33) / 32.0, np.arange(0, 19) / 18.0, [1e-7, -1e-7, 0.5 - 1e-7, 0.5 + 1e-7]]))
    vs = np.unique(np.concatenate([np.arange(1, 16) / 16.0, np.arange(1, 12) / 12.0, [1e-6, 1 - 1e-6]]))
    uu, vv = np.meshgrid(us, vs, indexing="ij")
    phi, theta = uu.ravel() * 2 * np.pi, vv.ravel() * np.pi
    loc = np.stack([np.sin(theta) * np.sin(phi), np.cos(theta), -np.sin(theta) * np.cos(phi)], axis=1)
    out += [_dirs(loc), _dirs(loc @ R.T)]
    return np.ascontiguousarray(np.concatenate(out))


def families(e, orc, osc):
    """{(mode, family letter, shape): queries} for one entry, and family C's parts by deciding input"""
    def oracle0(q):
        return oracle_eval(orc, osc, 0, q)
    a = family_a(e)
    b = family_b(e, oracle0, a)
    c = family_c(e, oracle0, a, b)
    fam = {(0, "A", -1): a, (0, "B", -1): b}
    if c:
        fam[(0, "C", -1)] = np.concatenate([c[k] for k in sorted(c)])
    if e.hit_shapes:
        q0 = np.concatenate([a[:12000], b[::3]] + ([fam[(0, "C", -1)][::5]] if c else []))
        o0 = oracle0(q0)
        emitter_shape = {"mixed": {1: 0, 2: 1, 3: 2}}.get(e.kind, {0: 0})    # picked emitter -> shape index
        for idx, shape in emitter_shape.items():
            pick = o0[:, INDEX] == idx
            fam[(1, "D", shape)] = family_d(e, lambda q, s=shape: oracle_eval(orc, osc, 1, q, s), shape, (q0[pick], o0[pick]))
    if e.env:
        fam[(2, "E", -1)] = family_e()
    return fam, c


# ------------------------------------------------------------------------------------------------ what the families reach (test_emitter_sweep_cpu.py)
def _sides(x, t, near=4e-7, absolute=False):
    """(below, on, above): how many of the compared values x lie below, on and above their threshold t, among those within near * |t| of it (a few float32 steps)"""
    with np.errstate(invalid="ignore"):
        x, t = np.asarray(x, F32), np.asarray(t, F32)
        tol = near if absolute else near * np.maximum(np.abs(t.astype(np.float64)), 1e-30)
        k = ~np.isnan(x) & ~np.isnan(t) & (np.abs(x.astype(np.float64) - t) <= tol)
        return int((k & (x < t)).sum()), int((k & (x == t)).sum()), int((k & (x > t)).sum())


def _search_sides(lo, hi, v):
    """a search that picks the first entry whose cdf is not < v: cdf[picked - 1] < v <= cdf[picked].  (below, on, above) = how often the entry before the picked one
    lies just below v, the picked one ON v, the picked one just above v"""
    return _sides(lo, v)[0], _sides(hi, v)[1], _sides(hi, v)[2]


def compares(e, fam, out):
    """{name of a compare of the emitter chain: (below, on, above)} over one entry's queries, from the operands orc_kat_emitter_n reports.  `near` keeps the count to
    queries that sit AT the threshold (a few float32 steps; 1e-6 around 0 for the cosines dp), so that a family that merely straddles it from afar does not count.
    Two entries are plain class counts, as their comments say."""
    o0 = np.concatenate([out[k] for k in sorted(fam) if k[0] == 0])
    res = {}
    if e.kind in ("spot", "mixed") and not np.isnan(o0[:, SCALED]).all():
        x = o0[:, SCALED]
        res["pick: e1 * ne against k"] = _sides(x, np.rint(x))
    if e.kind in ("mesh", "mixed"):
        v = o0[:, FACE_V]
        res["mesh: cdf[mid] < v"] = _search_sides(o0[:, CDF_LO], o0[:, CDF_HI], v)
    if e.kind.startswith("rect_bitmap"):
        res["texture: row search, cdf[mid] < v"] = _search_sides(o0[:, ROW_LO], o0[:, ROW_HI], o0[:, ROW_V])
        res["texture: column search, cdf[mid] < v"] = _search_sides(o0[:, COL_LO], o0[:, COL_HI], o0[:, COL_V])
    if e.kind == "envmap":
        for lv in range(3):
            res["envmap: level %d, sy > r0" % (lv + 1)] = _sides(o0[:, HIER + 4 * lv], o0[:, HIER + 4 * lv + 1])
            res["envmap: level %d, sx > c0" % (lv + 1)] = _sides(o0[:, HIER + 4 * lv + 2], o0[:, HIER + 4 * lv + 3])
    if e.kind == "spot":
        res["spot: cos_theta >= cos_beam"] = _sides(o0[:, COS_THETA], o0[:, COS_BEAM])
        res["spot: cos_theta > cos_cutoff"] = _sides(o0[:, COS_THETA], o0[:, COS_CUTOFF])
    if e.kind in ("sphere", "mixed"):
        res["sphere: dc_2 > sqr(radius_adj)"] = _sides(o0[:, DC2], o0[:, RADJ2])
        res["sphere: sin_theta_max_2 > 0.00068523"] = _sides(o0[:, STM2], np.full(len(o0), STM2_SWITCH))
    if e.kind in ("sphere", "mixed"):
        with np.errstate(invalid="ignore"):   # (how many: the reference point AT the centre; outside, at distance 0 from the sampled point; anything else)
            res["sphere: reference at the centre, dist == 0"] = (int((o0[:, DC2] == 0).sum()), int(((o0[:, DC2] > o0[:, RADJ2]) & (o0[:, DIST] == 0)).sum()), int((o0[:, DC2] > 0).sum()))
    if e.hit_shapes:
        z0 = np.zeros(len(o0), F32)
        res["area: dot(d, n) < 0 at the sampled point"] = _sides(o0[:, SAMPLE_DP], z0, 1e-6, absolute=True)
        with np.errstate(invalid="ignore"):
            # (how many: a density but not usable = back-facing; no density at all = coincident point or grazing, dist2 / dp not finite; usable)
            res["area: ds_pdf != 0 and facing"] = (int(((o0[:, USABLE] == 0) & (o0[:, PDF] > 0)).sum()), int((o0[:, PDF] == 0).sum()), int((o0[:, USABLE] == 1).sum()))
    for k in sorted(fam):
        if k[0] == 1:
            o1 = out[k]
            res["hit side, shape %d: dp < 0" % k[2]] = _sides(o1[:, DP], np.zeros(len(o1), F32), 1e-6, absolute=True)
            if e.kind == "sphere" or (e.kind == "mixed" and k[2] == 1):
                res["hit side, shape %d: sin_alpha < 0.99999994" % k[2]] = _sides(o1[:, SIN_ALPHA], np.full(len(o1), SIN_ALPHA_SWITCH))
    return res

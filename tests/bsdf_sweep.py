"""Inputs of the BSDF sweep (test_bsdf_sweep_cpu.py, test_bsdf_sweep_gpu.py): a catalogue of single-shape materials and five deterministic query families for
`bsdf_eval_pdf_sample`, the largest piece of float arithmetic on the path -- on the device through dtof_bsdf_eval_ex (every SPEC instantiation), in the oracle
through orc_kat_bsdf_n.  A query is 29 floats: wi[3], wo[3], sample1, sample2[2], uv[2], then dp_du, dp_dv, n, sh_s, sh_t, sh_n.

  A  random   unit wi / wo uniform on the sphere, samples and uv uniform in [0, 1), identity frame
  B  edges    z of wi and wo from +-0, denormals, ... +-1 (Z_EDGES) x four azimuths, sample1 from the constants of the catalogue, sample2 on the edge of the square
  C  thresholds   queries of A and B issued again with sample1 ON the value the oracle compared it with at a lobe choice (orc_kat_bsdf_n reports it), and on the
                  float below and above: the only inputs that tell `<` from `<=` in a lobe choice
  D  uv edges (textured materials)   u, v outside [0, 1], on texel centres and boundaries +- 1 ulp, far away
  E  frames (normalmap / bumpmap)    rotated, scaled, skewed and tilted interaction geometry x a subset of B and D

Unit vectors are built in float64 and rounded once.  Everything is a function of the seed."""
import ctypes as C
import os
import sys
from collections import namedtuple

import numpy as np

F32 = np.float32
ONE_BELOW = np.nextafter(F32(1), F32(0))
DENORMAL = np.nextafter(F32(0), F32(1))
TEX_W, TEX_H = 8, 4                      # the test images: not square, so that u and v cannot be swapped unnoticed
FLAT = np.array([1, 0, 0,  0, 1, 0,  0, 0, 1,  1, 0, 0,  0, 1, 0,  0, 0, 1], F32)   # dp_du, dp_dv, n, sh_s, sh_t, sh_n
N_A = 200000
SEED = 20240229

# ------------------------------------------------------------------------------------------------ the catalogue
SCENE = '<scene version="3.0.0"><shape type="rectangle">%s</shape></scene>'
DIFFUSE = '<bsdf type="diffuse"><rgb name="reflectance" value="0.2, 0.5, 0.8"/></bsdf>'
ETA_K = '<rgb name="eta" value="0.2, 0.92, 1.1"/><rgb name="k" value="3.9, 2.45, 2.14"/>'
CONDUCTOR = '<bsdf type="conductor">%s</bsdf>' % ETA_K
PLASTIC = '<bsdf type="plastic"><rgb name="diffuse_reflectance" value="0.1, 0.27, 0.36"/>%s</bsdf>'
ROUGHCONDUCTOR = '<bsdf type="roughconductor"><string name="distribution" value="ggx"/><float name="alpha" value="0.3"/>%s</bsdf>' % ETA_K


def _rough(kind, body):
    return '<bsdf type="%s">%s</bsdf>' % (kind, body)


def _distr(name, alpha="0.3"):
    return '<string name="distribution" value="%s"/><float name="alpha" value="%s"/>' % (name, alpha)


ALL_NORMALS = '<boolean name="sample_visible" value="false"/>'
RP = '<rgb name="diffuse_reflectance" value="0.5, 0.4, 0.3"/>'

# name, the <bsdf> element, the SPEC instantiations the render path can run on it, which wi let a lobe choice run (None: the chain has none), whether family D
# (a texture) and family E (a normalmap / bumpmap frame) apply
Material = namedtuple("Material", "name bsdf specs choice textured framed")
ANY, FRONT, BACK, NONZERO = "any", "front", "back", "nonzero"


def _bitmap(path, name=None, filt="bilinear", wrap="repeat"):
    return ('<texture type="bitmap"%s><string name="filename" value="%s"/><boolean name="raw" value="true"/><string name="filter_type" value="%s"/>'
            '<string name="wrap_mode" value="%s"/></texture>' % (' name="%s"' % name if name else "", path, filt, wrap))


def catalogue(texdir=""):
    """Every material of the sweep.  `texdir` holds the PNGs `write_textures` made (the names do not depend on it: catalogue() alone lists them)."""
    rgb, gray, normal = (os.path.join(texdir, n) for n in ("sweep_rgb.png", "sweep_gray.png", "sweep_normal.png"))
    m = []

    def add(name, bsdf, specs=(1, 2), choice=None, textured=False, framed=False):
        m.append(Material(name, bsdf, specs, choice, textured, framed))

    add("diffuse", DIFFUSE, (0, 1, 2))
    add("twosided_diffuse", '<bsdf type="twosided">%s</bsdf>' % DIFFUSE, (0, 1, 2))
    add("conductor", CONDUCTOR)
    add("twosided_conductor", '<bsdf type="twosided">%s</bsdf>' % CONDUCTOR)
    add("dielectric", '<bsdf type="dielectric"/>', choice=ANY)
    add("dielectric_inverted", '<bsdf type="dielectric"><float name="int_ior" value="1.0"/><float name="ext_ior" value="1.5"/></bsdf>', choice=ANY)
    add("dielectric_one_ulp", '<bsdf type="dielectric"><float name="int_ior" value="1.00000011920929"/><float name="ext_ior" value="1.0"/></bsdf>', choice=ANY)
    add("thindielectric", '<bsdf type="thindielectric"/>', choice=ANY)
    add("plastic", PLASTIC % "", choice=FRONT)
    add("plastic_nonlinear", PLASTIC % '<boolean name="nonlinear" value="true"/>', choice=FRONT)
    add("roughconductor_ggx", ROUGHCONDUCTOR)
    add("roughconductor_ggx_1e-4", _rough("roughconductor", _distr("ggx", "0.0001") + ETA_K))
    add("roughconductor_beckmann_aniso", _rough("roughconductor", '<string name="distribution" value="beckmann"/><float name="alpha_u" value="0.05"/>'
                                                                  '<float name="alpha_v" value="0.8"/>' + ETA_K))
    add("roughconductor_all_normals", _rough("roughconductor", _distr("ggx") + ALL_NORMALS + ETA_K))
    add("roughplastic_ggx", _rough("roughplastic", _distr("ggx", "0.25") + RP), choice=FRONT)
    add("roughplastic_beckmann", _rough("roughplastic", _distr("beckmann", "0.25") + RP), choice=FRONT)
    add("roughplastic_all_normals", _rough("roughplastic", _distr("ggx", "0.25") + ALL_NORMALS + RP), choice=FRONT)
    add("roughdielectric_ggx", _rough("roughdielectric", _distr("ggx")), choice=NONZERO)
    add("roughdielectric_beckmann", _rough("roughdielectric", _distr("beckmann")), choice=NONZERO)
    add("roughdielectric_all_normals", _rough("roughdielectric", _distr("ggx") + ALL_NORMALS), choice=NONZERO)
    add("roughdielectric_inverted", _rough("roughdielectric", _distr("ggx") + '<float name="int_ior" value="1.0"/><float name="ext_ior" value="1.5"/>'), choice=NONZERO)
    add("null", '<bsdf type="null"/>')
    # the mask's nested BSDF has a lobe choice of its own, so that the innermost comparison sees sample1 / opacity
    add("mask_0.3", '<bsdf type="mask"><float name="opacity" value="0.3"/>%s</bsdf>' % (PLASTIC % ""), choice=FRONT)
    add("mask_0", '<bsdf type="mask"><float name="opacity" value="0"/>%s</bsdf>' % DIFFUSE, choice=FRONT)
    add("mask_1", '<bsdf type="mask"><float name="opacity" value="1"/>%s</bsdf>' % DIFFUSE, choice=FRONT)
    blend = '<bsdf type="blendbsdf"><float name="weight" value="%s"/>' + DIFFUSE + ROUGHCONDUCTOR + '</bsdf>'
    add("blend_0.4", blend % "0.4", (2,), choice=FRONT)
    add("blend_0", blend % "0", (2,), choice=FRONT)
    add("blend_1", blend % "1", (2,), choice=FRONT)
    add("twosided_two_bsdfs", '<bsdf type="twosided">%s%s</bsdf>' % (DIFFUSE, PLASTIC % ""), (2,), choice=BACK)
    nm = '<bsdf type="normalmap">' + _bitmap(normal, "normalmap") + '%s</bsdf>'
    bm = '<bsdf type="bumpmap"><float name="scale" value="0.4"/>' + _bitmap(gray) + '%s</bsdf>'
    for tag, wrap in (("normalmap", nm), ("bumpmap", bm)):
        for inner_tag, inner in (("diffuse", DIFFUSE), ("roughconductor", ROUGHCONDUCTOR)):
            add("%s_%s" % (tag, inner_tag), wrap % inner, textured=True, framed=True)
            add("twosided_%s_%s" % (tag, inner_tag), '<bsdf type="twosided">%s</bsdf>' % (wrap % inner), textured=True, framed=True)
    for filt in ("nearest", "bilinear"):
        for wrap in ("repeat", "mirror", "clamp"):
            t = "%s_%s" % (filt, wrap)
            add("bitmap_reflectance_" + t, '<bsdf type="diffuse">%s</bsdf>' % _bitmap(rgb, "reflectance", filt, wrap), textured=True)
            add("bitmap_specular_reflectance_" + t, PLASTIC % _bitmap(rgb, "specular_reflectance", filt, wrap), choice=FRONT, textured=True)
            add("bitmap_alpha_" + t, _rough("roughconductor", '<string name="distribution" value="ggx"/>' + _bitmap(rgb, "alpha", filt, wrap) + ETA_K), textured=True)
            add("bitmap_opacity_" + t, '<bsdf type="mask">%s%s</bsdf>' % (_bitmap(gray, "opacity", filt, wrap), DIFFUSE), choice=FRONT, textured=True)
            add("bitmap_weight_" + t, '<bsdf type="blendbsdf">%s%s%s</bsdf>' % (_bitmap(gray, "weight", filt, wrap), DIFFUSE, ROUGHCONDUCTOR), (2,), choice=FRONT, textured=True)
    add("bitmap_normal_bilinear_clamp", '<bsdf type="normalmap">%s%s</bsdf>' % (_bitmap(normal, "normalmap", "bilinear", "clamp"), DIFFUSE), textured=True, framed=True)
    add("checkerboard_reflectance", '<bsdf type="diffuse"><texture type="checkerboard" name="reflectance"><rgb name="color0" value="0.1, 0.2, 0.3"/>'
                                    '<rgb name="color1" value="0.9, 0.8, 0.7"/></texture></bsdf>', textured=True)
    return m


NAMES = [m.name for m in catalogue()]
CONSTANTS = [0.3, 0.4]                   # every constant opacity and weight of the catalogue that is not 0 or 1 (those are in the grid anyway)


def write_textures(texdir):
    """The three TEX_W x TEX_H test images: RGB without 0 / 255 (it also feeds `alpha`), gray with both (opacities and weights of exactly 0 and 1), and normals
    tilted up to ~40 degrees."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenes"))
    import make_scenes
    texdir = str(texdir)
    make_scenes.write_png(os.path.join(texdir, "sweep_rgb.png"), [[(16 + (x * 37 + y * 91) % 224, 16 + (x * 59 + y * 23 + 7) % 224, 16 + (x * 13 + y * 101 + 50) % 224)
                                                                  for x in range(TEX_W)] for y in range(TEX_H)])
    gray = [[(x * 67 + y * 29 + 3) % 256 for x in range(TEX_W)] for y in range(TEX_H)]
    gray[0][0], gray[1][3], gray[2][5], gray[3][7] = 0, 255, 0, 255
    make_scenes.write_png(os.path.join(texdir, "sweep_gray.png"), gray)
    rows = []
    for y in range(TEX_H):
        row = []
        for x in range(TEX_W):
            tilt, phi = np.radians(5 + 35 * ((x * 3 + y * 5) % 8) / 7.0), 2 * np.pi * ((x * 5 + y * 3) % 11) / 11.0
            n = np.array([np.sin(tilt) * np.cos(phi), np.sin(tilt) * np.sin(phi), np.cos(tilt)])
            row.append(tuple(int(v) for v in np.clip(np.round((n * 0.5 + 0.5) * 255), 0, 255)))
        rows.append(row)
    make_scenes.write_png(os.path.join(texdir, "sweep_normal.png"), rows)
    return texdir


# ------------------------------------------------------------------------------------------------ the families
Z_EDGES = np.array([0.0, -0.0, DENORMAL, -DENORMAL, 2.0 ** -126, -2.0 ** -126, 1e-20, -1e-20, 1e-6, -1e-6, 1e-3, -1e-3, 0.1, -0.1, 0.5, 0.9, ONE_BELOW, 1.0, -1.0], F32)
AZIMUTHS = [0.0, 1.1, 2.9, 4.6]
S2_MAX = 1.0 - 2.0 ** -24
S2_EDGES = np.array([(x, y) for x in (0.0, 0.5, S2_MAX) for y in (0.0, 0.5, S2_MAX)] + [(1e-8, 1e-8)], F32)
S1_EDGES = np.array([0.0, ONE_BELOW, 0.5] + CONSTANTS + [1.0], F32)


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)


def edge_directions():
    """z from Z_EDGES x AZIMUTHS: (sqrt(1 - z^2) cos phi, sqrt(1 - z^2) sin phi, z) in float64, rounded once; z itself arrives unchanged"""
    z = Z_EDGES.astype(np.float64)
    r = np.sqrt(1.0 - z * z)
    d = np.array([[r[i] * np.cos(p), r[i] * np.sin(p), z[i]] for i in range(len(z)) for p in AZIMUTHS]).astype(F32)
    d[:, 2] = np.repeat(Z_EDGES, len(AZIMUTHS))      # keeps the sign of -0
    return d


def _with_frame(q11, frame=FLAT):
    return np.ascontiguousarray(np.concatenate([np.asarray(q11, F32), np.broadcast_to(np.asarray(frame, F32), (len(q11), 18))], axis=1))


def family_a(n=N_A, seed=SEED):
    rng = np.random.default_rng(seed)
    q = np.empty((n, 11), F32)
    q[:, 0:3] = _unit(rng.standard_normal((n, 3)))
    q[:, 3:6] = _unit(rng.standard_normal((n, 3)))
    q[:, 6:11] = rng.random((n, 5), dtype=F32)
    return _with_frame(q)


def family_b(seed=SEED):
    """wi x wo x sample1 with sample2 cycling through its edge set, then wi x sample1 x sample2 with wo cycling: every pair of the crossed axes meets"""
    d = edge_directions()
    rng = np.random.default_rng(seed + 1)
    nd, n1, n2 = len(d), len(S1_EDGES), len(S2_EDGES)
    i, j, k = np.meshgrid(np.arange(nd), np.arange(nd), np.arange(n1), indexing="ij")
    i, j, k = i.ravel(), j.ravel(), k.ravel()
    first = np.concatenate([d[i], d[j], S1_EDGES[k, None], S2_EDGES[(i * 7 + j * 3 + k) % n2]], axis=1)
    i, k, l = np.meshgrid(np.arange(nd), np.arange(n1), np.arange(n2), indexing="ij")
    i, k, l = i.ravel(), k.ravel(), l.ravel()
    second = np.concatenate([d[i], d[(i * 5 + k * 11 + l * 3) % nd], S1_EDGES[k, None], S2_EDGES[l]], axis=1)
    q = np.concatenate([first, second]).astype(F32)
    return _with_frame(np.concatenate([q, rng.random((len(q), 2), dtype=F32)], axis=1))


def uv_edges():
    vals = [-1.25, -1.0, -2.0 ** -24, 0.0, -0.0, 2.0 ** -24, 0.5, ONE_BELOW, 1.0, 1.0 + 2.0 ** -23, 2.5, 1e6, -1e6]
    for res in (TEX_W, TEX_H):
        for t in range(2 * res + 1):       # texel boundaries (even t) and centres (odd t) of the test images
            x = F32(t / (2.0 * res))
            vals += [np.nextafter(x, F32(-1)), x, np.nextafter(x, F32(2))]
    return np.unique(np.array(vals, F32).view(np.uint32)).view(F32)      # by bit pattern: keeps +0 and -0 apart


def family_d(seed=SEED):
    """every (u, v) of uv_edges() with directions and samples drawn from family A's distribution, two per texture coordinate pair"""
    e = uv_edges()
    u, v = np.meshgrid(e, e, indexing="ij")
    uv = np.repeat(np.stack([u.ravel(), v.ravel()], axis=1), 2, axis=0)
    q = family_a(len(uv), seed + 2)
    q[:, 9:11] = uv
    return q


def frames():
    """(name, 18 floats) of family E: the interaction geometry normalmap / bumpmap build their frames from"""
    def rot(axis, deg):
        a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a); t = np.radians(deg)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K
    I = np.eye(3)
    out = [("identity", FLAT.astype(np.float64))]
    R = rot([1, 2, 3], 50.0)                                   # columns: the images of x, y, z
    out.append(("rotated", np.concatenate([R[:, 0], R[:, 1], R[:, 2], R[:, 0], R[:, 1], R[:, 2]])))
    for name, s in (("scaled_1e-3", 1e-3), ("scaled_1e3", 1e3)):
        out.append((name, np.concatenate([I[0] * s, I[1] * s, I[2], I[0], I[1], I[2]])))
    c, s = np.cos(np.radians(60.0)), np.sin(np.radians(60.0))
    out.append(("skewed_60", np.concatenate([[c, s, 0], I[1], I[2], I[0], I[1], I[2]])))
    T = rot([1, 0, 0], 20.0)
    out.append(("shading_normal_tilted_20", np.concatenate([I[0], I[1], I[2], T[:, 0], T[:, 1], T[:, 2]])))
    return [(n, f.astype(F32)) for n, f in out]


def family_e(b, d):
    """each frame x every 7th query of B and every 5th of D"""
    sub = np.concatenate([b[::7, :11], d[::5, :11]])
    return np.concatenate([_with_frame(sub, f) for _, f in frames()])


def lets_a_choice_run(material, q):
    z = q[:, 2]
    return {ANY: np.ones(len(q), bool), FRONT: z > 0, BACK: z < 0, NONZERO: z != 0, None: np.zeros(len(q), bool)}[material.choice]


def _neighbours(x, k=4):
    """x and its k float32 neighbours on each side, nearest first: (n, 2k + 1)"""
    x = np.asarray(x, F32)
    cols, lo, hi = [x], x, x
    for _ in range(k):
        lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
        cols += [lo, hi]
    return np.stack(cols, axis=1)


def compared_value(level, s1, opacity, weight):
    """What the chain compares with its level's threshold when given sample1 = s1, in the oracle's own float32 operations (mask: sample1 itself; blend: sample1 /
    opacity under a mask; innermost: that, rescaled by the blend's sample1 / w or (sample1 - w) / (1 - w)).  NaN opacity / weight = no such adapter."""
    with np.errstate(all="ignore"):
        x = np.asarray(s1, F32)
        if level >= 1:
            x = np.where(np.isnan(opacity), x, x / opacity).astype(F32)
        if level == 2:
            x = np.where(np.isnan(weight), x, np.where(x <= weight, x / weight, (x - weight) / (F32(1) - weight))).astype(F32)
    return x


LEVELS = ("mask opacity", "blend weight", "innermost choice")
Thresholds = namedtuple("Thresholds", "q triple role level target missing")   # role: -1 / 0 / +1 = the compared value is the float below / on / above `target`


def family_c(material, a, b, oracle, n_a=6000, n_b=2000):
    """`oracle`: (n, 29) -> (n, 17).  For the first n_a queries of A and n_b of B whose wi lets a lobe choice run, and each lobe choice that ran: the query with
    sample1 mapped back through the outer rescalings so that the compared value is the threshold, the float below and the float above.  The back-mapping is done in
    float64 and the 9 float32 values around it are searched for one whose compared value (compared_value) lands exactly; `missing` counts the ones that have none."""
    base = np.concatenate([a[lets_a_choice_run(material, a)][:n_a], b[lets_a_choice_run(material, b)][:n_b]])
    if not len(base):
        return Thresholds(np.zeros((0, 29), F32), np.zeros(0, np.int64), np.zeros(0, np.int8), np.zeros(0, np.int8), np.zeros(0, F32), 0)
    thr = oracle(base)[:, 14:17]
    opacity, weight = thr[:, 0].copy(), thr[:, 1].copy()
    qs, triple, role, level, target, missing, n_triples = [], [], [], [], [], 0, 0
    for lv in range(3):
        rows = np.nonzero(~np.isnan(thr[:, lv]))[0]
        if not len(rows):
            continue
        t, op, w = thr[rows, lv], opacity[rows], weight[rows]
        with np.errstate(all="ignore"):
            for r, goal in ((-1, np.nextafter(t, F32(-np.inf))), (0, t), (1, np.nextafter(t, F32(np.inf)))):
                x = goal.astype(np.float64)
                if lv == 2:      # the side of the blend the base query picked is the one whose threshold was reported
                    side_1 = compared_value(1, base[rows, 6], op, w) <= w
                    x = np.where(np.isnan(w), x, np.where(side_1, x * w, x * (1.0 - w) + w))
                if lv >= 1:
                    x = np.where(np.isnan(op), x, x * op)
                cand = _neighbours(np.nan_to_num(x, nan=0.0, posinf=3e38, neginf=-3e38).astype(F32))
                hit = compared_value(lv, cand, op[:, None], w[:, None]).view(np.uint32) == goal.view(np.uint32)[:, None]
                found = hit.any(axis=1)
                s1 = cand[np.arange(len(rows)), hit.argmax(axis=1)]
                q = base[rows[found]].copy()
                q[:, 6] = s1[found]
                qs.append(q); triple.append(n_triples + np.nonzero(found)[0]); role.append(np.full(len(q), r, np.int8))
                level.append(np.full(len(q), lv, np.int8)); target.append(t[found]); missing += int((~found).sum())
        n_triples += len(rows)
    return Thresholds(np.concatenate(qs), np.concatenate(triple), np.concatenate(role), np.concatenate(level), np.concatenate(target), missing)


def families(material, oracle):
    """{family letter: (n, 29) queries} for one material, and family C's bookkeeping"""
    a, b = family_a(), family_b()
    c = family_c(material, a, b, oracle)
    out = {"A": a, "B": b, "C": c.q}
    if material.textured:
        out["D"] = family_d()
    if material.framed:
        out["E"] = family_e(b, out["D"])
    return out, c


# ------------------------------------------------------------------------------------------------ both sides
def oracle_eval(orc, shape, q29):
    """orc_kat_bsdf_n: (n, 29) -> (n, 17): the 14 outputs of dtof_bsdf_eval_ex, then the thresholds of the three lobe choices (NaN: did not run)"""
    q = np.ascontiguousarray(q29, F32).reshape(-1, 29)
    out = np.zeros((len(q), 17), F32)
    orc.lib().orc_kat_bsdf_n(C.byref(shape), len(q), q.ctypes.data, out.ctypes.data)
    return out


CANARY = 0x7FA5C3D2      # a NaN no arithmetic produces


def device_eval(mi, scene, spec, q29, shape_index=0):
    """dtof_bsdf_eval_ex into a buffer pre-filled with CANARY: returns (return code, (n, 14) output as uint32)"""
    q = np.ascontiguousarray(q29, F32).reshape(-1, 29)
    out = np.full((len(q), 14), CANARY, np.uint32)
    rc = mi._lib().dtof_bsdf_eval_ex(scene._h, shape_index, spec, len(q), q.ctypes.data, out.ctypes.data)
    return rc, out


def same_bits(x, y):
    """elementwise: equal as bit patterns, two NaNs equal whatever their payload"""
    x, y = np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)
    return (x == y) | (np.isnan(x.view(F32)) & np.isnan(y.view(F32)))


OUTPUT_WORDS = ("value.r", "value.g", "value.b", "pdf", "wo.x", "wo.y", "wo.z", "sample pdf", "eta", "delta", "weight.r", "weight.g", "weight.b", "null")


def describe_mismatch(material, family, q, got, want, what="device vs oracle"):
    """the failure message: material, family, the first five differing queries with all inputs in hex, and which output words differ"""
    bad = ~same_bits(got, want)
    rows = np.nonzero(bad.any(axis=1))[0]
    lines = ["%s, family %s, %s: %d of %d queries differ" % (material, family, what, len(rows), len(q))]
    for r in rows[:5]:
        lines.append("  query %d in = %s" % (r, " ".join("%08x" % w for w in np.ascontiguousarray(q[r]).view(np.uint32))))
        for c in np.nonzero(bad[r])[0]:
            lines.append("    %-10s got %08x want %08x" % (OUTPUT_WORDS[c], np.asarray(got[r]).view(np.uint32)[c], np.asarray(want[r]).view(np.uint32)[c]))
    return "\n".join(lines)

"""The queries of the surface-interaction sweep (tests/surface_sweep.py) are what test_surface_sweep_gpu.py needs, shown on the oracle alone: every discrete decision
compute_si and offset_p make is met on each side of its compare and on its value in every scene that has it; the reachable family reproduces the ray query's own
records; and the rows that are NaN -- where two answers are equal whatever they hold -- stay a small share."""
import ctypes as C

import numpy as np
import pytest

import surface_sweep as ss


@pytest.fixture(scope="module")
def sweeps(orc, tmp_path_factory):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ss.Sweep(name, orc, tmp_path_factory.mktemp(name))
        return cache[name]
    return get


def _kinds(sw):
    return {s.kind for s in sw.slots}


@pytest.mark.parametrize("name", ss.NAMES)
def test_every_decision_is_met_on_each_side_and_on_its_value(sweeps, name):
    sw = sweeps(name)
    ops, kinds = sw.ops, _kinds(sw)
    col = lambda k: ops[:, ss.OPS.index(k)]      # noqa: E731
    tiny = float(np.finfo(np.float32).tiny)
    if ss.DISK in kinds:
        # r = sqrt(b2 b2 + b1 b1) is a square root: never below 0, and never a denormal either -- the smallest positive argument, 2^-149, has the root 2^-74.5, a
        # normal float, so rcp(r) cannot overflow for r != 0.  Met: on 0 (with zero and with non-zero operands), the smallest r above it, and r on / around 1.
        r = col("disk_r")
        disk = ~np.isnan(r)
        nonzero = disk & ((sw.q[:, 8] != 0) | (sw.q[:, 9] != 0))
        assert (r[disk] == 0).any() and (r[nonzero] == 0).any() and (r[disk] > 0).any() and not (r[disk] < 0).any()
        assert ((r[disk] > 0) & (r[disk] < tiny)).sum() == 0 and r[disk & (r > 0)].min() < 1e-22
        assert (r[disk] == 1).any() and ((r[disk] < 1) & (r[disk] > 0.99)).any() and (r[disk] > 1).any()
    if ss.SPHERE in kinds:
        rd = col("sphere_rd")      # a square root as well: on 0 (the poles of the sphere placed for it) and above
        sph = ~np.isnan(rd)
        assert (rd[sph] == 0).any() and (rd[sph] > 0).any() and not (rd[sph] < 0).any()
        assert ((rd[sph] > 0) & (rd[sph] < 1e-3)).any(), "no query beside a pole"
    if name == "mesh":
        det = col("mesh_det")      # a constant of the face, not of the query: the edge mesh brings each side, the value and a denormal
        has = ~np.isnan(det)
        assert (det[has] < 0).any() and (det[has] == 0).any() and (det[has] > 0).any() and ((det[has] > 0) & (det[has] < tiny)).any()
        # ... and the vertex normals that cancel: the interpolated normal is the zero vector on the row built for it, one float either side it is not
        edge = [s for s in sw.slots if s.kind == ss.MESH and s.n_faces == 5][0]
        rows = np.flatnonzero((sw.ids[:, 0] == edge.obj) & (sw.ids[:, 2] == 2) & (sw.q[:, 9] == 0))
        at = {float(sw.q[i, 8]): np.isnan(sw.want[i, ss.SH_N]).all() for i in rows}
        assert at[0.5] and not at[ss.fl(ss.step(0.5, 1))] and not at[ss.fl(ss.step(0.5, -1))]
    zero = col("dpdu_zero")
    assert (zero == 0).any()
    if ss.CYL in kinds or name == "wall_mirror":      # the cylinder's axis; the mirrored wall at the shutter's middle.  Elsewhere no input makes dp_du the zero vector:
        assert (zero == 1).any()                       # a rectangle's and a disk's are columns of an invertible matrix, a triangle's an edge or a tangent of unit length
    w = col("weight")
    moving = ~np.isnan(w)
    assert moving.any() and (col("segment")[moving] == 0).all()      # (every scene has its instance; keyframes 0 and 1 are the only segment)
    time = sw.q[:, 6]
    assert ((w == 0) & (time < 0)).any() and ((w == 0) & (time == 0)).any() and ((w > 0) & (w < 1e-3)).any(), "the lower clamp: below, on, above"
    assert ((w == 1) & (time > ss.SHUTTER)).any() and ((w == 1) & (time == np.float32(ss.SHUTTER))).any() and ((w < 1) & (w > 0.999)).any(), "the upper clamp"
    dot = col("offset_dot")
    assert (dot < 0).any() and (dot > 0).any() and ((dot == 0) & np.signbit(dot)).any() and ((dot == 0) & ~np.signbit(dot)).any()
    pos = np.abs(dot[(dot != 0) & ~np.isnan(dot)])
    assert pos.min() < 1e-6, "no query beside dot(n, d) == 0"


@pytest.mark.parametrize("name", ss.NAMES)
def test_the_reachable_family_reproduces_the_ray_querys_records(sweeps, orc, name):
    sw = sweeps(name)
    a = np.flatnonzero(sw.family == "A")
    unreached = {(s.obj, s.k) for s in sw.slots} - {(int(i), int(k)) for i, k in sw.ids[a, :2]}
    # every shape of the scene is reached -- but for the doubled rectangles of the two tie scenes, which lose every tie to their twin: no ray query reports them, and
    # they are rows of B and C alone (a hit is given, not traced)
    assert len(a) >= 1000 and len(unreached) == (2 if name in ("ties", "ties_wall") else 0), unreached
    placed = {(int(i), int(k)) for i, k in sw.ids[sw.family == "B", :2]}
    assert unreached <= placed
    L = orc.lib()
    out, ids = np.zeros(25, np.float32), np.zeros(3, np.int32)
    for j, i in enumerate(a):
        r = sw.rays_a[j]
        o, d = np.ascontiguousarray(r[0:3]), np.ascontiguousarray(r[3:6])
        assert L.orc_kat_ray_intersect(C.byref(sw.osc.c), o.ctypes.data, d.ctypes.data, C.c_float(float(r[6])), C.c_float(float(r[7])), out.ctypes.data, ids.ctypes.data) == 1
        # t, p, n, sh_n, sh_s, sh_t, dp_du, dp_dv, wi
        mine = np.concatenate([sw.q[i, 7:8], sw.want[i, 0:15], sw.want[i, ss.DP_DU], sw.want[i, ss.DP_DV], sw.want[i, ss.WI]])
        assert np.array_equal(ids, sw.ids[i]) and np.array_equal(mine.view(np.uint32), out.view(np.uint32)), (name, int(i))


@pytest.mark.parametrize("name", ss.NAMES)
def test_the_nan_share_is_capped(sweeps, name):
    sw = sweeps(name)
    in_a, share = sw.nan_share()
    fam, cnt = np.unique(sw.family, return_counts=True)
    print("%s: %d rows (%s); rows with a NaN word: %d in A, %.2f %% of B and C" % (name, sw.n, ", ".join("%s %d" % fc for fc in zip(fam, cnt)), in_a, 100 * share))
    assert in_a == 0
    # ... which holds because reachable hits with a NaN word are rows of B: they lie on the ONE face built to be NaN, the edge mesh's face 1 (det = 1e-40, an
    # infinite dp_du), and nowhere else -- a NaN on an ordinary reachable hit fails here
    moved = sw.moved_out_of_a
    if name == "mesh":
        edge = [s for s in sw.slots if s.kind == ss.MESH and s.n_faces == 5][0]
        assert len(moved) > 0 and (moved[:, 0] == edge.obj).all() and (moved[:, 1] == edge.k).all() and (moved[:, 2] == 1).all(), moved
    else:
        assert len(moved) == 0, moved
    assert share <= ss.NAN_CAP
    b = sw.family == "B"
    assert sw.nan_rows()[b].mean() < 0.10, "the rows built to be NaN stay below one row in ten of B"
    assert sw.n <= 50000
    # the inputs themselves are finite but for the rows that say otherwise on purpose (none here)
    assert np.isfinite(sw.q).all()


def test_the_tangent_negates_the_rounded_dot_product(sweeps):
    """Regression, found by the device sweep: initialize_sh_frame (interaction.h:259-260) is fmadd(n, -dot(n, dp_du), dp_du) with the negation applied to the rounded
    dot product.  Where the dot's products cancel to a zero, folding the negation into its last multiply-add gives the zero of the other sign, and the components of
    sh_s in which n_i * 0 meets a zero of dp_du flip theirs.  The two rows that showed it, with the signs worked out by hand: a face of the rotated cube
    (n = (-0.5, 0, -0.866), dp_du = (-0, -0.5, 0): dot = +0, s.x = fma(-0.5, -0, -0) = +0) and the disk hit on its local x axis."""
    for name, ids, q, word, negative in (
            ("mesh", (4, 0, 11), ((-3.638639211654663, 3.034635543823242, -1.5972764492034912), (3.646522283554077, -4.448401927947998, 1.4039480686187744), 0.0,
                                  0.9715331196784973, 0.567152202129364, 0.07426836341619492), 9, False),
            ("analytic", (4, 0, 0), ((3.9612503051757812, -2.3658978939056396, -1.9264013767242432), (-2.7519264221191406, 4.2604522705078125, 2.2753517627716064),
                                     0.0010563131654635072, 0.8975040912628174, -2.6469782757140506e-23, 0.0), 11, False)):
        sw = sweeps(name)
        out = sw.answer(ss.row(*q), ids)[0][0]
        assert out[word] == 0 and bool(np.signbit(out[word])) == negative, (name, out[ss.SH_N], out[ss.DP_DU], out[ss.SH_S])

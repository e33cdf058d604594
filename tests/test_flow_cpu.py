"""World-to-pixel matrices and the flow of static geometry under a moving camera (dtof_scene_world_to_pixel, Scene.world_to_pixel, harness.camera_flow), none of
which needs a device:
  - the header declares and the library exports the entry; its refusals
  - S against numpy: the matrix built in float64 from dtof_scene_export kind 2 and the film size, for a perspective, a thinlens and an orthographic sensor (the last
    with the scale in to_world that sets its extent) and a cropped film; tolerance 2^-40 of the largest entry, the project's bound for double results -- the depth row
    is absent, so no near / far conditioning enters
  - an independent hold on S and on its coordinates: pix(p) of every ORACLE lane's own hit position (orc_kat_ray_intersect on the lanes of render_lanes) is the
    lane's sample_pos, for the perspective and the orthographic sensor, with and without a crop window
  - camera_flow: equal sensors give +-0, a sideways step of the camera gives the closed form, points behind a camera give NaN
  - the flow film's entries (dtof_render_flow, dtof_sample_flow_lanes): declared and exported, refused like the aov film's before any device call with nothing
    written, DTOF_ERR_HIP without a device; the nine reference aov types are not extended."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aov_ref as A  # noqa: E402
import test_sensors as TS  # noqa: E402

CROP = ('<integer name="crop_offset_x" value="5"/><integer name="crop_offset_y" value="3"/><integer name="crop_width" value="9"/><integer name="crop_height" value="7"/>'
        '<rfilter type="tent"/>')
SENSORS = {"perspective": TS.scene_text("perspective", ""), "thinlens": TS.scene_text(), "orthographic": TS.ortho_text(),
           "perspective, cropped": TS.scene_text("perspective", "").replace('<rfilter type="tent"/>', CROP),
           "orthographic, cropped": TS.ortho_text().replace('<rfilter type="tent"/>', CROP)}
FILM_W, FILM_H = 24, 16


def numpy_S(export2, film_w, film_h):
    """rows x, y, w of camera_to_sample o to_world^-1 in film pixels (include/mitsuba/render/sensor.h:226-299), float64"""
    e = np.asarray(export2, np.float64)
    V = np.linalg.inv(e[:16].reshape(4, 4))
    aspect = film_w / film_h
    if e[21] == 2.0:      # orthographic
        proj = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 0, 1.0]])
    else:
        cot = 1.0 / np.tan(np.float64(np.float32(e[16]) * np.float32(0.5)) * (np.pi / 180.0))
        proj = np.array([[cot, 0, 0, 0], [0, cot, 0, 0], [0, 0, 1.0, 0]])
    shift = np.array([[1.0, 0, -1.0], [0, 1.0, -1.0 / aspect], [0, 0, 1.0]])
    scale = np.diag([-0.5 * film_w, -0.5 * aspect * film_h, 1.0])
    return scale @ shift @ proj @ V


def pix(S, p):
    p1 = np.concatenate([np.asarray(p, np.float64), np.ones((len(p), 1))], axis=1)
    return (p1 @ S[:2].T) / (p1 @ S[2])[:, None]


def test_header_declares_and_library_exports_the_entry(mi):
    hdr = open(os.path.join(ROOT, "include", "dtof.h")).read()
    assert re.search(r"\bint\s+dtof_scene_world_to_pixel\s*\(const dtof_scene \*scene, double out12\[12\]\)\s*;", hdr)
    assert hasattr(C.CDLL(mi.lib_path()), "dtof_scene_world_to_pixel")
    L = mi._lib()
    assert L.dtof_scene_world_to_pixel.argtypes == [C.c_void_p, C.c_void_p]
    sc = mi.load_string(SENSORS["perspective"])
    out = np.full(12, 7.0)
    assert L.dtof_scene_world_to_pixel(None, out.ctypes.data) == 1 and L.dtof_scene_world_to_pixel(sc._h, None) == 1 and (out == 7.0).all()
    no_sensor = mi.load_string('<scene version="3.0.0"><shape type="rectangle"/></scene>')
    assert L.dtof_scene_world_to_pixel(no_sensor._h, out.ctypes.data) == 1 and b"sensor" in L.dtof_last_error() and (out == 7.0).all()
    with pytest.raises(mi.DtofError, match="sensor"):
        no_sensor.world_to_pixel()


@pytest.mark.parametrize("name", list(SENSORS))
def test_world_to_pixel_against_numpy(mi, name):
    sc = mi.load_string(SENSORS[name])
    S = sc.world_to_pixel()
    assert S.shape == (3, 4) and S.dtype == np.float64
    want = numpy_S(sc.export(2), FILM_W, FILM_H)
    err = np.abs(S - want).max()
    print("%s: largest entry %.6g, largest difference %.3g = 2^%.1f of it" % (name, np.abs(want).max(), err, np.log2(max(err, 5e-324) / np.abs(want).max())))
    assert err <= 2.0 ** -40 * np.abs(want).max()
    if name.startswith("orthographic"):
        assert (S[2] == [0.0, 0.0, 0.0, 1.0]).all()
    else:
        assert np.abs(S[2, :3]).max() > 0.1      # the camera's viewing direction


@pytest.mark.parametrize("name", ["perspective", "orthographic", "perspective, cropped", "orthographic, cropped"])
def test_every_oracle_hit_projects_onto_its_sample_position(mi, orc, name):
    """The hold that touches neither the formula above nor a kernel: the oracle's camera ray through sample_pos hits the scene at p, so pix(p) must be sample_pos --
    in FILM pixels, also under a crop window.  What separates the two is the float32 rounding of the ray and of the hit: |p| <= 8 carries 2^-21 of a unit at most,
    the ray's direction as much over t <= 8, and the film has under 10 pixels per unit at the rectangle (24 pixels across 2 x 6 tan 15 deg = 3.2 units), i.e. about
    1e-5 pixels; 1e-3 is the bound.  Measured: 3.5e-6 (perspective), 2.1e-6 (orthographic), 1.8e-6 and 1.6e-6 pixels under the crop."""
    osc = orc.Scene(SENSORS[name], is_string=True)
    lanes = A.ref.lanes_of(orc, osc, osc.params(), 3, 8)
    out25, ids = A.intersect(orc, osc, lanes)
    hit = A.check_far_plane(osc, out25, ids)
    assert hit.sum() > len(hit) // 4
    S = mi.load_string(SENSORS[name]).world_to_pixel()
    dev = np.abs(pix(S, out25[hit, 1:4]) - np.asarray(lanes["sample_pos"], np.float64)[hit])
    print("%s: %d hits, largest |pix(p) - sample_pos| %.3g pixels" % (name, int(hit.sum()), dev.max()))
    assert dev.max() < 1e-3
    if "cropped" in name:      # film coordinates: the crop window's pixels, not 0 .. crop size
        pos = np.asarray(lanes["sample_pos"])
        assert pos[:, 0].min() >= 4 and pos[:, 0].max() <= 15 and pos[:, 1].min() >= 2 and pos[:, 1].max() <= 11


def test_camera_flow(mi):
    from mitsuba3dopplertof_amd import harness
    text = SENSORS["perspective"]
    S = mi.load_string(text).world_to_pixel()
    rng = np.random.default_rng(2)
    position = np.stack([rng.uniform(-1.5, 1.5, (5, 7)), rng.uniform(-1.5, 1.5, (5, 7)), rng.uniform(-0.5, 0.5, (5, 7))], axis=2)
    flow = harness.camera_flow(position, S, S)
    assert flow.shape == (5, 7, 2) and flow.dtype == np.float32 and (flow == 0).all()
    # the camera steps sideways by 0.1 along its own x axis: a point at depth z moves by (-0.5 film_w) cot (-0.1) / z pixels in x and not at all in y
    e = np.asarray(mi.load_string(text).export(2), np.float64)
    to_world = e[:16].reshape(4, 4)
    step = 0.1 * to_world[:3, 0]
    moved = text.replace('<lookat origin="0.5, 1, 6" target="0, 0.5, 0" up="0, 1, 0"/>',
                         '<lookat origin="%.17g, %.17g, %.17g" target="%.17g, %.17g, %.17g" up="0, 1, 0"/>' % (tuple(np.array([0.5, 1, 6]) + step) + tuple(np.array([0, 0.5, 0]) + step)))
    S_cur = mi.load_string(moved).world_to_pixel()
    flow = harness.camera_flow(position, S, S_cur)
    p1 = np.concatenate([position, np.ones((5, 7, 1))], axis=2)
    z = p1 @ np.linalg.inv(to_world)[2]
    cot = 1.0 / np.tan(np.radians(15.0))
    assert (z > 4).all()
    assert np.allclose(flow[..., 0], 0.5 * FILM_W * cot * 0.1 / z, rtol=1e-4) and np.abs(flow[..., 1]).max() < 1e-4
    behind = position.copy()
    behind[2, 3] = to_world[:3, 3] - 2.0 * to_world[:3, 2]      # two units behind the first camera
    flow = harness.camera_flow(behind, S, S_cur)
    assert np.isnan(flow[2, 3]).all() and np.isfinite(np.delete(flow.reshape(-1, 2), 2 * 7 + 3, axis=0)).all()


def test_flow_entries_are_declared_refuse_and_have_no_cpu_fallback(mi):
    import subprocess
    from conftest import SCENES
    hdr = open(os.path.join(ROOT, "include", "dtof.h")).read()
    lib = C.CDLL(mi.lib_path())
    for name in ("dtof_render_flow", "dtof_sample_flow_lanes"):
        assert re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr) and hasattr(lib, name), name
    L = mi._lib()
    vp = C.c_void_p
    assert L.dtof_render_flow.argtypes[:6] == [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, vp]
    assert L.dtof_sample_flow_lanes.argtypes == [vp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, vp, vp]
    # the nine reference aov types are not extended: the flow film is no aov type
    assert "flow" not in mi.AOV_TYPES and len(mi.AOV_TYPES) == 9
    with pytest.raises(mi.DtofError):
        mi.aov_channels("f:flow")
    wall = os.path.join(SCENES, "cornell_wall.xml")
    sc = mi.load_file(wall, resx=8, resy=8)
    planes, lanes, flow = np.full((3, 8, 8), 7.0), np.full((4, 12), 7.0, np.float32), np.full((4, 2), 7.0, np.float32)
    assert L.dtof_render_flow(None, 0, 4, 1, 1, planes.ctypes.data, None) == 1 and L.dtof_render_flow(sc._h, 0, 4, 1, 1, None, None) == 1
    assert L.dtof_render_flow(sc._h, 0, 4, 0, 1, planes.ctypes.data, None) == 1 and b"at least one pass" in L.dtof_last_error()
    assert L.dtof_sample_flow_lanes(None, 0, 4, 0, 4, lanes.ctypes.data, flow.ctypes.data) == 1
    assert L.dtof_sample_flow_lanes(sc._h, 0, 4, 0, 4, None, flow.ctypes.data) == 1 and L.dtof_sample_flow_lanes(sc._h, 0, 4, 0, 4, lanes.ctypes.data, None) == 1
    no_sensor = mi.load_string('<scene version="3.0.0"><shape type="rectangle"/></scene>')
    assert L.dtof_render_flow(no_sensor._h, 0, 4, 1, 1, planes.ctypes.data, None) == 1 and b"sensor" in L.dtof_last_error()
    assert (planes == 7.0).all() and (lanes == 7.0).all() and (flow == 7.0).all()
    child = ("import sys, numpy as np\nsys.path.insert(0, sys.argv[1])\nimport mitsuba3dopplertof_amd as mi\nsc = mi.load_file(sys.argv[2], resx=8, resy=8)\n"
             "L = mi._lib()\np, a, f = np.full((3, 8, 8), 7.0), np.zeros((4, 12), np.float32), np.zeros((4, 2), np.float32)\n"
             "print(L.dtof_render_flow(sc._h, 0, 4, 1, 1, p.ctypes.data, None), L.dtof_sample_flow_lanes(sc._h, 0, 4, 0, 4, a.ctypes.data, f.ctypes.data), int((p == 7.0).all()))")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", child, ROOT, wall], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.split() == ["2", "2", "1"], (r.stdout, r.stderr[-2000:])

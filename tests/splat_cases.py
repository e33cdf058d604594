"""The case matrix of the float32 splat tests, shared by test_splat_cpu.py (the criterion holds on the oracle's own float32 film, and sees every mutation) and
test_splat_gpu.py (the device's films).  Every case: cornell_wall.xml with one filter, one frame, one sample count; the kernel and shape Scene.last_splat must report
are written down here from the kernels' description in csrc/dtof_kernels.hip, and tests/splat_choice_check.cpp holds the function that chooses them."""
import os

from conftest import SCENES

SEED = 4
K4 = [(0.0, 0.0), (0.0, 0.25), (1.0, 0.0), (1.0, 0.25)]

TENT = '<rfilter type="tent" />'
FILTERS = {
    "tent": TENT,
    "box": '<rfilter type="box" />',
    "gaussian": '<rfilter type="gaussian" />',                                                          # stddev 0.5, radius 2: 5 x 5
    "gaussian_narrow": '<rfilter type="gaussian"><float name="stddev" value="0.25" /></rfilter>',       # radius 1: 3 x 3
    "mitchell": '<rfilter type="mitchell" />',                                                          # radius 2, negative lobes
    "catmullrom": '<rfilter type="catmullrom" />',
    "tent2": '<rfilter type="tent"><float name="radius" value="2.0" /></rfilter>',
    "tent2.5": '<rfilter type="tent"><float name="radius" value="2.5" /></rfilter>',                    # reach 2, the widest x8 takes
    "tent2.6": '<rfilter type="tent"><float name="radius" value="2.6" /></rfilter>',                    # reach 3: 7 x 7
    "tent0.5": '<rfilter type="tent"><float name="radius" value="0.5" /></rfilter>',                    # reach 0: one tap, weighted
    "lanczos": '<rfilter type="lanczos" />',                                                            # 3 lobes: 7 x 7, negative lobes
}
FORMAT = '<string name="file_format"'

# frames: name -> (-D parameters, crop (x, y, w, h) or None).  "far": a 16 x 12 window at (32768, 16384) of a 32784 x 16396 film -- sample positions beyond 2^15
# have an 8-bit fraction, so a jitter close to 1 rounds to the next integer: IRREGULAR samples, whose float position floors into the next pixel.  "far_y": the
# window at (32768, 32768), as many of them along y; "far_wide": 48 x 40 pixels there.  The window's last column or row holds some, whose footprint then leaves
# the window.  (The pixel kernel runs at 48 spp there: 4 parts of 12, and as many irregular samples as 64 spp would give x8.)
FRAMES = {
    "16x12": (dict(resx=16, resy=12), None),
    "17x13": (dict(resx=17, resy=13), None),
    "8x6": (dict(resx=8, resy=6), None),
    "crop": (dict(resx=32, resy=24), (5, 3, 16, 12)),
    "far": (dict(resx=32784, resy=16396), (32768, 16384, 16, 12)),
    "far_y": (dict(resx=32784, resy=32780), (32768, 32768, 16, 12)),
    "far_wide": (dict(resx=32816, resy=32808), (32768, 32768, 48, 40)),      # k_splat_tent3 runs at 8 spp at most: more pixels for as many irregular samples
}


def x8(n, seg8):
    return {"kernel": "x8", "n": n, "seg8": seg8}


def pixel(n, parts, chunk):
    return {"kernel": "pixel", "n": n, "parts": parts, "chunk": chunk}


def tent3(seg):
    return {"kernel": "tent3", "n": 3, "seg": seg}


def generic(n):
    return {"kernel": "generic", "n": n}


FUSED = {"kernel": "fused", "n": 3}
NO_FUSE = {"DTOF_FUSE_SPLAT": "0"}


def case(filt, frame, spp, want, K=1, rgba=False, env=None, rows=None):
    return dict(filter=filt, frame=frame, spp=spp, want=want, K=K, rgba=rgba, env=env or {}, rows=rows)


CASES = {
    # ---- k_splat_x8: every seg8 (each switches on one more DPP step), two segments a pixel at 1024 spp
    "x8_tent@16": case("tent", "16x12", 16, x8(3, 2)),
    "x8_tent@32": case("tent", "16x12", 32, x8(3, 4)),
    "x8_tent@64": case("tent", "16x12", 64, x8(3, 8), env=NO_FUSE),
    "x8_tent@128": case("tent", "16x12", 128, x8(3, 16)),
    "x8_tent@256": case("tent", "16x12", 256, x8(3, 32)),
    "x8_tent@512": case("tent", "8x6", 512, x8(3, 64)),
    "x8_tent@1024": case("tent", "8x6", 1024, x8(3, 64)),
    "x8_box@16": case("box", "16x12", 16, x8(1, 2)),
    "x8_box@128": case("box", "16x12", 128, x8(1, 16)),
    "x8_gaussian_narrow@32": case("gaussian_narrow", "16x12", 32, x8(3, 4)),
    "x8_gaussian@16": case("gaussian", "16x12", 16, x8(5, 2)),
    "x8_mitchell@32": case("mitchell", "16x12", 32, x8(5, 4)),
    "x8_catmullrom@64": case("catmullrom", "16x12", 64, x8(5, 8)),
    "x8_tent2@256": case("tent2", "16x12", 256, x8(5, 32)),
    "x8_tent2.5@16": case("tent2.5", "16x12", 16, x8(5, 2)),
    "x8_tent@64_K4": case("tent", "16x12", 64, x8(3, 8), K=4),                       # four films never fuse; the `k > 0` barrier
    "x8_gaussian@16_K4": case("gaussian", "16x12", 16, x8(5, 2), K=4),
    "x8_box@16_rgba": case("box", "16x12", 16, x8(1, 2), rgba=True),
    "x8_tent@32_rgba": case("tent", "16x12", 32, x8(3, 4), rgba=True),
    "x8_gaussian@16_rgba": case("gaussian", "16x12", 16, x8(5, 2), rgba=True),
    # ---- the splat fused into k_shade: 64 spp, radius-1 tent, one film, default switches
    "fused_tent@64": case("tent", "16x12", 64, FUSED),
    "fused_tent@64_far": case("tent", "far", 64, FUSED),
    # ---- k_splat_pixel on 17 x 13 (221 threads per part: no multiple of 64): parts 1; 2 (9 + 8); 2 (12 + 12); 4 (9, 9, 9, 6); 8 (chunk 13, last 9)
    "pixel_tent@3": case("tent", "17x13", 3, pixel(3, 1, 3)),
    "pixel_box@5": case("box", "17x13", 5, pixel(1, 1, 5)),
    "pixel_gaussian@12": case("gaussian", "17x13", 12, pixel(5, 1, 12)),
    "pixel_tent@17": case("tent", "17x13", 17, pixel(3, 2, 9)),
    "pixel_mitchell@24_rgba": case("mitchell", "17x13", 24, pixel(5, 2, 12), rgba=True),
    "pixel_gaussian@33": case("gaussian", "17x13", 33, pixel(5, 4, 9)),
    "pixel_box@33": case("box", "17x13", 33, pixel(1, 4, 9)),
    "pixel_tent@100": case("tent", "17x13", 100, pixel(3, 8, 13)),
    "pixel_mitchell@100": case("mitchell", "17x13", 100, pixel(5, 8, 13)),
    "pixel_tent@17_K4": case("tent", "17x13", 17, pixel(3, 2, 9), K=4),
    "pixel_tent@1": case("tent", "16x12", 1, pixel(3, 1, 1)),                        # one sample a pixel: one thread per pixel, not the per-lane kernel
    # ---- k_splat_tent3
    "tent3_tent@2": case("tent", "16x12", 2, tent3(2)),
    "tent3_tent@4": case("tent", "16x12", 4, tent3(4)),
    "tent3_tent@8": case("tent", "16x12", 8, tent3(8)),
    "tent3_tent@4_K4": case("tent", "16x12", 4, tent3(4), K=4),
    "tent3_tent@8_K4": case("tent", "17x13", 8, tent3(8), K=4),
    # ---- k_splat_generic
    "generic_lanczos@4": case("lanczos", "16x12", 4, generic(7)),
    "generic_tent0.5@4": case("tent0.5", "16x12", 4, generic(1)),
    "generic_tent2.6@4": case("tent2.6", "16x12", 4, generic(7)),
    "generic_tent@16_switch": case("tent", "16x12", 16, generic(3), env={"DTOF_SPLAT": "generic"}),
    "generic_lanczos@16_K4": case("lanczos", "17x13", 16, generic(7), K=4),
    # ---- placement, for x8, pixel and tent3 each: a crop window, the irregular-sample frame, a row band, batches of three rows with a last batch of one
    "x8_tent@16_crop": case("tent", "crop", 16, x8(3, 2)),
    "x8_tent@64_far": case("tent", "far", 64, x8(3, 8), env=NO_FUSE),
    "x8_gaussian@64_far_y": case("gaussian", "far_y", 64, x8(5, 8)),
    "x8_tent@16_band": case("tent", "17x13", 16, x8(3, 2), rows=(5, 9)),
    "x8_tent@16_batches": case("tent", "17x13", 16, x8(3, 2), env={"DTOF_BATCH_LANES": "1000"}),
    "pixel_tent@12_crop": case("tent", "crop", 12, pixel(3, 1, 12)),
    "pixel_tent@48_far_y": case("tent", "far_y", 48, pixel(3, 4, 12)),
    "pixel_gaussian@48_far_y": case("gaussian", "far_y", 48, pixel(5, 4, 12)),
    "pixel_tent@12_band": case("tent", "17x13", 12, pixel(3, 1, 12), rows=(5, 9)),
    "pixel_tent@17_batches": case("tent", "17x13", 17, pixel(3, 2, 9), env={"DTOF_BATCH_LANES": "1000"}),      # 289 lanes a row: three rows per batch, the last has one
    "tent3_tent@8_crop": case("tent", "crop", 8, tent3(8)),
    "tent3_tent@8_far_wide": case("tent", "far_wide", 8, tent3(8)),
    "tent3_tent@8_band": case("tent", "17x13", 8, tent3(8), rows=(5, 9)),
    "tent3_tent@8_batches": case("tent", "17x13", 8, tent3(8), env={"DTOF_BATCH_LANES": "500"}),               # 136 lanes a row: three rows per batch, the last has one
}
# irregular lanes a far frame must hold per axis at the sample count its case runs with (test_splat_cpu.test_the_irregular_sample_frames)
FAR_MIN = 8


def scene_xml(c):
    xml = open(os.path.join(SCENES, "cornell_wall.xml")).read()
    assert TENT in xml and FORMAT in xml
    xml = xml.replace(TENT, FILTERS[c["filter"]])
    params, crop = FRAMES[c["frame"]]
    if crop:
        xml = xml.replace(FORMAT, '<integer name="crop_offset_x" value="%d" /><integer name="crop_offset_y" value="%d" /><integer name="crop_width" value="%d" />'
                          '<integer name="crop_height" value="%d" />' % crop + FORMAT)
    if c["rgba"]:
        old = '<string name="pixel_format" value="rgb" />'
        assert old in xml
        xml = xml.replace(old, '<string name="pixel_format" value="rgba" />')
    params = dict(params)
    if c["spp"] % 2:
        params["time_sampling_method"] = "uniform"
    return xml, params


def variants(c):
    return K4 if c["K"] == 4 else None
